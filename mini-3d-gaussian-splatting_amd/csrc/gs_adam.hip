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

// ================================================ Adam on visible rows =====
// One launch for all tensors: block b -> (tensor, kRowBlock consecutive rows)
// through the same prefix table.  The block stages its rows' mask bytes in
// LDS and leaves before any load of p, g, m or v when none is set; a live
// block streams its rows' elements as float4 (kRowBlock is a multiple of 4:
// the block's first element row0 * cols is 16-B aligned when the bases are)
// and skips the float4s none of whose elements belongs to a visible row.
constexpr int kRowBlock = GS_ADAM_ROW_BLOCK;
static_assert(kRowBlock % 4 == 0 && kRowBlock % kBlock == 0, "rows per block: whole float4s, whole mask rounds");
// the row of a block-relative element e is umulhi(e, magic), exact while
// e * cols < 2^32; e < kRowBlock * cols
static_assert((uint64_t)kRowBlock * GS_ADAM_ROWS_MAX_COLS * GS_ADAM_ROWS_MAX_COLS < (1ull << 32), "multiply-high range");

// adam_update where `on`; the old bits (whatever g holds) otherwise
__device__ __forceinline__ void adam_update_if(bool on, float &p, float &m, float &v, float g, float om1, float b2,
                                               float om2, float step, float bc2s, float eps) {
  float pn = p, mn = m, vn = v;
  adam_update(pn, mn, vn, g, om1, b2, om2, step, bc2s, eps);
  p = on ? pn : p;
  m = on ? mn : m;
  v = on ? vn : v;
}

__global__ __launch_bounds__(kBlock) void k_adam_rows(gs_adam_rows_args a, int4 firsts0, int4 firsts1, uint4 magic0,
                                                      uint4 magic1) {
  __shared__ uint8_t s_mask[kRowBlock];
  const int starts[GS_ADAM_MAX_TENSORS + 1] = {firsts0.x, firsts0.y, firsts0.z, firsts0.w,
                                               firsts1.x, firsts1.y, firsts1.z, firsts1.w, 0x7fffffff};
  const uint32_t magics[GS_ADAM_MAX_TENSORS] = {magic0.x, magic0.y, magic0.z, magic0.w,
                                                magic1.x, magic1.y, magic1.z, magic1.w};
  int ti = 0;
#pragma unroll
  for (int k = 1; k < GS_ADAM_MAX_TENSORS; ++k) ti += (int)blockIdx.x >= starts[k] ? 1 : 0;
  const gs_adam_tensor &t = a.adam.t[ti];
  if (!t.grad) return;
  const int64_t row0 = (int64_t)(blockIdx.x - starts[ti]) * kRowBlock;
  const int nrows = (int)min((int64_t)kRowBlock, a.rows - row0);
  // the block's mask bytes: one coalesced read (bytes: the mask may start
  // anywhere, a range of rows hands in an offset pointer)
  int any = 0;
#pragma unroll
  for (int k = 0; k < kRowBlock / kBlock; ++k) {
    const int r = k * kBlock + (int)threadIdx.x;
    const uint8_t on = r < nrows ? (a.row_mask[row0 + r] != 0) : 0;
    s_mask[r] = on;
    any |= on;
  }
  if (!__syncthreads_or(any)) return;  // (block-uniform: no row of the block is visible)

  uint32_t cols = 0, magic = 0;
#pragma unroll
  for (int k = 0; k < GS_ADAM_MAX_TENSORS; ++k) {  // (constant indices: the tables stay in scalar registers)
    cols = k == ti ? (uint32_t)a.cols[k] : cols;
    magic = k == ti ? magics[k] : magic;
  }
  const int64_t first = row0 * cols;
  float *const P = t.param + first, *const M = t.exp_avg + first, *const V = t.exp_avg_sq + first;
  const float *const G = t.grad + first;
  const uint32_t E = (uint32_t)nrows * cols;  // the block's elements
  const float b2 = a.adam.beta2, om1 = a.adam.one_minus_beta1, om2 = a.adam.one_minus_beta2, eps = a.adam.eps;
  const float step = t.lr / t.bias_correction1, bc2s = t.bias_correction2_sqrt;
  const bool vec = ((reinterpret_cast<uintptr_t>(P) | reinterpret_cast<uintptr_t>(G) | reinterpret_cast<uintptr_t>(M) |
                     reinterpret_cast<uintptr_t>(V)) & 15) == 0;
  const uint32_t E4 = vec ? (E & ~3u) : 0u;
  for (uint32_t e0 = threadIdx.x * 4u; e0 < E4; e0 += kBlock * 4u) {
    // the rows of the float4's elements: one multiply-high, then counting
    uint32_t r = cols == 1 ? e0 : __umulhi(e0, magic);
    uint32_t rem = e0 - r * cols;
    bool on[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      on[k] = s_mask[r] != 0;
      if (++rem == cols) {
        rem = 0;
        ++r;  // (past the block's last row only after the last element)
      }
    }
    if (!(on[0] | on[1] | on[2] | on[3])) continue;
    float4 p = *reinterpret_cast<const float4 *>(P + e0);
    const float4 g = *reinterpret_cast<const float4 *>(G + e0);
    float4 m = *reinterpret_cast<const float4 *>(M + e0);
    float4 v = *reinterpret_cast<const float4 *>(V + e0);
    adam_update_if(on[0], p.x, m.x, v.x, g.x, om1, b2, om2, step, bc2s, eps);
    adam_update_if(on[1], p.y, m.y, v.y, g.y, om1, b2, om2, step, bc2s, eps);
    adam_update_if(on[2], p.z, m.z, v.z, g.z, om1, b2, om2, step, bc2s, eps);
    adam_update_if(on[3], p.w, m.w, v.w, g.w, om1, b2, om2, step, bc2s, eps);
    *reinterpret_cast<float4 *>(P + e0) = p;
    *reinterpret_cast<float4 *>(M + e0) = m;
    *reinterpret_cast<float4 *>(V + e0) = v;
  }
  // misaligned bases, and the up to three elements after the last float4
  for (uint32_t e = E4 + threadIdx.x; e < E; e += kBlock) {
    const uint32_t r = cols == 1 ? e : __umulhi(e, magic);
    if (!s_mask[r]) continue;
    float p = P[e], m = M[e], v = V[e];
    adam_update(p, m, v, G[e], om1, b2, om2, step, bc2s, eps);
    M[e] = m;
    V[e] = v;
    P[e] = p;
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

gs_status gs_adam_step_rows(const gs_adam_rows_args *a, gs_stream_t stream) {
  const char *const fn = "gs_adam_step_rows";
  if (!a || a->adam.num_tensors < 0 || a->adam.num_tensors > GS_ADAM_MAX_TENSORS || !a->row_mask || a->rows < 0)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: bad args (null args or row_mask, rows < 0, num_tensors)", fn);
  if (a->adam.skip_flag || a->adam.hyper || a->adam.hyper_row)
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: skip_flag / hyper / hyper_row are not supported", fn);
  int starts[GS_ADAM_MAX_TENSORS] = {0};
  uint32_t magic[GS_ADAM_MAX_TENSORS] = {0};
  const long long row_blocks = (a->rows + kRowBlock - 1) / kRowBlock;
  long long nblk = 0;
  bool too_wide = false;
  for (int i = 0; i < GS_ADAM_MAX_TENSORS; ++i) {
    starts[i] = (int)(nblk < 0x7fffffffLL ? nblk : 0x7fffffffLL);
    if (i >= a->adam.num_tensors) continue;
    const gs_adam_tensor &t = a->adam.t[i];
    if (!t.grad) continue;
    if (!t.param || !t.exp_avg || !t.exp_avg_sq)
      return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", fn);
    if (a->cols[i] < 1 || t.numel != a->rows * (int64_t)a->cols[i])
      return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: every tensor with a grad needs cols >= 1 and numel == rows * cols", fn);
    if (t.param_out) return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: param_out is not supported", fn);
    too_wide |= a->cols[i] > GS_ADAM_ROWS_MAX_COLS;
    magic[i] = (uint32_t)((1ull << 32) / (uint32_t)a->cols[i] + 1);  // (cols 1 wraps to 1: the kernel does not use it)
    nblk += row_blocks;
  }
  if (too_wide) return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: cols above GS_ADAM_ROWS_MAX_COLS", fn);
  if (nblk == 0) return GS_OK;
  if (nblk > 0x7fffffffLL) return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: too many rows", fn);
  gs_adam_rows_args c = *a;
  c.adam.one_minus_beta1 = one_minus_beta(c.adam.one_minus_beta1, c.adam.beta1);
  c.adam.one_minus_beta2 = one_minus_beta(c.adam.one_minus_beta2, c.adam.beta2);
  for (int i = a->adam.num_tensors; i < GS_ADAM_MAX_TENSORS; ++i) c.adam.t[i].grad = nullptr;
  k_adam_rows<<<(unsigned)nblk, kBlock, 0, (hipStream_t)stream>>>(
      c, make_int4(starts[0], starts[1], starts[2], starts[3]), make_int4(starts[4], starts[5], starts[6], starts[7]),
      make_uint4(magic[0], magic[1], magic[2], magic[3]), make_uint4(magic[4], magic[5], magic[6], magic[7]));
  return gs_internal_check_launch(fn);
}

}  // extern "C"
