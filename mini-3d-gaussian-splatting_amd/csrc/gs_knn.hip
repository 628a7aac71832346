// gs_knn.hip -- exact k-nearest-neighbour search over a point cloud
// (include/gsplat_mi355x.h, "k-nearest neighbours"): simple_knn's distCUDA2,
// the start-up scale of every 3DGS trainer.
//
// The result is defined without reference to the search: row i is the k
// smallest pairs (d2(p_i, p_j), j), j != i, in lexicographic order, d2 the one
// function below.  The search -- Morton order (60 bits, in two sorts of 30),
// boxes of 256 consecutive points, AABB culls -- only decides which pairs are
// never looked at, and a pair is passed over only when a lower bound of its d2
// is strictly above the k-th best already held (see d2).  So the bits are the
// same on every run, every rank and every input order.  No atomics, no host
// read: a fixed launch sequence on the caller's stream.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gs_device.h"
#include "gs_internal.h"
#include "gsplat_mi355x.h"

namespace {

constexpr int kBox = kBlock;             // points per box: one query per lane of the workgroup
constexpr int kNear = 8;                 // boxes on either side in Morton order visited first
constexpr int32_t kMaxPoints = 1 << 30;  // sorted positions and box * 256 + lane stay in int32
constexpr int kNoRow = 0x7fffffff;       // an empty slot's row: after every real one

// The only place a distance is computed.  Fixed order, no contraction (the
// library is built with -ffp-contract=off): ((dx dx) + (dy dy)) + (dz dz) of
// the fp32 differences.
//
// The two culls call it too, on a point of the box that is at least as close
// per axis as any real one:
//   point to AABB:  d2(q, clamp(q, lo, hi))
//   AABB to AABB:   d2(a, b), per axis (a, b) = (lo_b, hi_q) if lo_b > hi_q,
//                   (lo_q, hi_b) if lo_q > hi_b, else (0, 0)
// Per axis the exact gap is no larger in magnitude than the exact difference
// to any point p of the box (to any pair q, p of the two boxes).  fp32
// subtraction, squaring and addition of non-negative terms are monotone, so
// the computed bound is <= the computed d2 to every such point, with no
// epsilon.  A box is passed over only when bound > threshold, strictly: on
// equality a smaller row at the same distance would displace the k-th.  This
// is the whole correctness argument; Morton quantisation, box size and the
// visiting order affect only speed.
__device__ __forceinline__ float d2(float ax, float ay, float az, float bx, float by, float bz) {
  const float dx = ax - bx, dy = ay - by, dz = az - bz;
  return (dx * dx + dy * dy) + dz * dz;
}

__device__ __forceinline__ float point_box_bound(const float4 &q, const float4 &lo, const float4 &hi) {
  return d2(q.x, q.y, q.z, fminf(fmaxf(q.x, lo.x), hi.x), fminf(fmaxf(q.y, lo.y), hi.y),
            fminf(fmaxf(q.z, lo.z), hi.z));
}

__device__ __forceinline__ void axis_gap(float lo_q, float hi_q, float lo_b, float hi_b, float &a, float &b) {
  a = b = 0.f;
  if (lo_b > hi_q) {
    a = lo_b;
    b = hi_q;
  } else if (lo_q > hi_b) {
    a = lo_q;
    b = hi_b;
  }
}
__device__ __forceinline__ float box_box_bound(const float4 &lo_q, const float4 &hi_q, const float4 &lo_b,
                                               const float4 &hi_b) {
  float ax, ay, az, bx, by, bz;
  axis_gap(lo_q.x, hi_q.x, lo_b.x, hi_b.x, ax, bx);
  axis_gap(lo_q.y, hi_q.y, lo_b.y, hi_b.y, ay, by);
  axis_gap(lo_q.z, hi_q.z, lo_b.z, hi_b.z, az, bz);
  return d2(ax, ay, az, bx, by, bz);
}

// ---------------------------------------------------- block min / max ----
// min and max of three floats per thread over the workgroup (s: 4 x 6 floats);
// every thread gets them.  min / max do not depend on the order: no atomics
// needed for the same bits every run.
__device__ __forceinline__ void block_minmax3(float (&lo)[3], float (&hi)[3], float (*s)[6]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      lo[c] = fminf(lo[c], __shfl_xor(lo[c], d, 64));
      hi[c] = fmaxf(hi[c], __shfl_xor(hi[c], d, 64));
    }
  }
  if (lane == 0) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      s[wave][c] = lo[c];
      s[wave][3 + c] = hi[c];
    }
  }
  __syncthreads();
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    lo[c] = fminf(fminf(s[0][c], s[1][c]), fminf(s[2][c], s[3][c]));
    hi[c] = fmaxf(fmaxf(s[0][3 + c], s[1][3 + c]), fmaxf(s[2][3 + c], s[3][3 + c]));
  }
  __syncthreads();
}

// level 1 of the cloud's bounding box: one (lo, hi) per 256 input rows
__global__ __launch_bounds__(kBlock) void k_knn_bbox_blocks(const float *__restrict__ points, int n, float4 *part) {
  __shared__ float s[kBlock / kWave][6];
  const int i = blockIdx.x * kBlock + threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n) {
#pragma unroll
    for (int c = 0; c < 3; ++c) lo[c] = hi[c] = points[3 * (size_t)i + c];
  }
  block_minmax3(lo, hi, s);
  if (threadIdx.x == 0) {
    part[2 * (size_t)blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.f);
    part[2 * (size_t)blockIdx.x + 1] = make_float4(hi[0], hi[1], hi[2], 0.f);
  }
}

// level 2: one workgroup over the nb partials
__global__ __launch_bounds__(kBlock) void k_knn_bbox_final(const float4 *__restrict__ part, int nb, float4 *bbox) {
  __shared__ float s[kBlock / kWave][6];
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int b = threadIdx.x; b < nb; b += kBlock) {
    const float4 l = part[2 * (size_t)b], h = part[2 * (size_t)b + 1];
    lo[0] = fminf(lo[0], l.x), lo[1] = fminf(lo[1], l.y), lo[2] = fminf(lo[2], l.z);
    hi[0] = fmaxf(hi[0], h.x), hi[1] = fmaxf(hi[1], h.y), hi[2] = fmaxf(hi[2], h.z);
  }
  block_minmax3(lo, hi, s);
  if (threadIdx.x == 0) {
    bbox[0] = make_float4(lo[0], lo[1], lo[2], 0.f);
    bbox[1] = make_float4(hi[0], hi[1], hi[2], 0.f);
  }
}

// ------------------------------------------------------------ Morton ----
__device__ __forceinline__ uint32_t spread10(uint32_t v) {  // bit i of 10 -> bit 3 i
  v = (v | (v << 16)) & 0x030000FFu;
  v = (v | (v << 8)) & 0x0300F00Fu;
  v = (v | (v << 4)) & 0x030C30C3u;
  v = (v | (v << 2)) & 0x09249249u;
  return v;
}
// 20 bits of an axis over the cloud's box; an axis of no (or no finite) extent gives 0
__device__ __forceinline__ uint32_t quantise20(float x, float lo, float hi) {
  const float ext = hi - lo;
  if (!(ext > 0.f) || isinf(ext)) return 0u;
  const float t = ((x - lo) / ext) * 1048576.f;
  return (uint32_t)min(1048575, max(0, (int)t));  // (speed only: any key gives the same result)
}

// The 60-bit Morton key of a point as two 30-bit words (the upper and the lower
// 10 bits of each axis): the cloud is ordered by two stable sorts, the low word
// first.  10 bits an axis over the whole box would leave a dense part of an SfM
// cloud -- half the points in 1 % of the volume -- unordered inside a few
// cells, its boxes of 256 each as wide as the cell.
__global__ __launch_bounds__(kBlock) void k_knn_morton(const float *__restrict__ points, int n,
                                                       const float4 *__restrict__ bbox, uint32_t *keys_lo,
                                                       uint32_t *keys_hi) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i >= n) return;
  const float4 lo = bbox[0], hi = bbox[1];
  const uint32_t qx = quantise20(points[3 * (size_t)i], lo.x, hi.x);
  const uint32_t qy = quantise20(points[3 * (size_t)i + 1], lo.y, hi.y);
  const uint32_t qz = quantise20(points[3 * (size_t)i + 2], lo.z, hi.z);
  keys_lo[i] = spread10(qx & 1023u) | (spread10(qy & 1023u) << 1) | (spread10(qz & 1023u) << 2);
  keys_hi[i] = spread10(qx >> 10) | (spread10(qy >> 10) << 1) | (spread10(qz >> 10) << 2);
}

// the second sort's keys: the high words in the first sort's order
__global__ __launch_bounds__(kBlock) void k_knn_high_keys(const uint32_t *__restrict__ keys_hi,
                                                          const uint32_t *__restrict__ order, int n, uint32_t *keys) {
  const int i = blockIdx.x * kBlock + threadIdx.x;
  if (i < n) keys[i] = keys_hi[order[i]];
}

// the points in sorted order as (x, y, z, row-as-bits), and each box's AABB
__global__ __launch_bounds__(kBlock) void k_knn_gather(const float *__restrict__ points, int n,
                                                       const uint32_t *__restrict__ order, float4 *sorted,
                                                       float4 *box_lo, float4 *box_hi) {
  __shared__ float s[kBlock / kWave][6];
  const int i = blockIdx.x * kBox + threadIdx.x;
  float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
  if (i < n) {
    const uint32_t row = order[i];
#pragma unroll
    for (int c = 0; c < 3; ++c) lo[c] = hi[c] = points[3 * (size_t)row + c];
    sorted[i] = make_float4(lo[0], lo[1], lo[2], __uint_as_float(row));
  }
  block_minmax3(lo, hi, s);
  if (threadIdx.x == 0) {
    box_lo[blockIdx.x] = make_float4(lo[0], lo[1], lo[2], 0.f);
    box_hi[blockIdx.x] = make_float4(hi[0], hi[1], hi[2], 0.f);
  }
}

// ------------------------------------------------------------ search ----
// (d, j) before (bd, bj) in the result's order
__device__ __forceinline__ bool before(float d, int j, float bd, int bj) { return d < bd || (d == bd && j < bj); }

// The K best of a query, ascending, in registers (every index is a
// compile-time constant after unrolling); the first k <= K slots are the
// result, (kd, kj) is slot k - 1.
template <int K>
struct Best {
  float d[K];
  int j[K];
  float kd;
  int kj;
  __device__ __forceinline__ void init() {
#pragma unroll
    for (int s = 0; s < K; ++s) {
      d[s] = INFINITY;
      j[s] = kNoRow;
    }
    kd = INFINITY;
    kj = kNoRow;
  }
  // a candidate before slot k - 1: into the last slot, then up to its place
  __device__ __forceinline__ void insert(float cd, int cj, int k) {
    d[K - 1] = cd;
    j[K - 1] = cj;
#pragma unroll
    for (int s = K - 1; s > 0; --s) {
      const bool sw = before(d[s], j[s], d[s - 1], j[s - 1]);
      const float td = d[s];
      const int tj = j[s];
      d[s] = sw ? d[s - 1] : td;
      j[s] = sw ? j[s - 1] : tj;
      d[s - 1] = sw ? td : d[s - 1];
      j[s - 1] = sw ? tj : j[s - 1];
    }
    kd = d[0];
    kj = j[0];
#pragma unroll
    for (int s = 1; s < K; ++s) {
      if (s < k) {
        kd = d[s];
        kj = j[s];
      }
    }
  }
};

// the largest v of the workgroup (s: 4 floats); ends in a barrier
__device__ __forceinline__ float block_max(float v, float *s) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = fmaxf(v, __shfl_xor(v, d, 64));
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  return fmaxf(fmaxf(s[0], s[1]), fmaxf(s[2], s[3]));
}

template <int K>
__global__ __launch_bounds__(kBlock) void k_knn_search(gs_knn_args a, const float4 *__restrict__ sorted,
                                                       const float4 *__restrict__ box_lo,
                                                       const float4 *__restrict__ box_hi, int nb) {
  __shared__ float4 s_pts[kBox];
  __shared__ float4 s_q[kBox];  // the sweep's copy of the queries: (x, y, z, k-th best)
  __shared__ float s_r2[kBlock / kWave];
  __shared__ unsigned long long s_mask[kBlock / kWave];
  const int b = blockIdx.x, t = threadIdx.x, n = a.n, k = a.k;
  const int qi = b * kBox + t;
  const bool valid = qi < n;
  const float4 q = sorted[valid ? qi : b * kBox];
  const float4 lo_q = box_lo[b], hi_q = box_hi[b];
  Best<K> best;
  best.init();

  // the query box's own points: every one but the query itself
  const int own = min(kBox, n - b * kBox);
  if (valid) s_pts[t] = q;
  __syncthreads();
  if (valid) {
    for (int c = 0; c < own; ++c) {
      const float4 p = s_pts[c];
      const float d = d2(q.x, q.y, q.z, p.x, p.y, p.z);
      const int j = __float_as_int(p.w);
      if (c != t && before(d, j, best.kd, best.kj)) best.insert(d, j, k);
    }
  }
  // the workgroup's cull radius: the largest k-th best among its queries
  float R2 = block_max(valid ? best.kd : -INFINITY, s_r2);

  // One box: passed over if its AABB is strictly farther from the query box
  // than R2; else staged in LDS, and every query whose own bound does not
  // exceed its own k-th best tests its points.  R2 is re-reduced after it.
  // (box, R2 and so every branch around a barrier are uniform.)
  auto visit = [&](int box) {
    box = __builtin_amdgcn_readfirstlane(box);
    const float4 lo = box_lo[box], hi = box_hi[box];
    if (box_box_bound(lo_q, hi_q, lo, hi) > R2) return;
    const int cnt = min(kBox, n - box * kBox);
    if (t < cnt) s_pts[t] = sorted[(size_t)box * kBox + t];
    __syncthreads();
    if (valid && !(point_box_bound(q, lo, hi) > best.kd)) {
      for (int c = 0; c < cnt; ++c) {
        const float4 p = s_pts[c];  // (every lane the same address: one broadcast read)
        const float d = d2(q.x, q.y, q.z, p.x, p.y, p.z);
        const int j = __float_as_int(p.w);
        if (before(d, j, best.kd, best.kj)) best.insert(d, j, k);
      }
    }
    R2 = block_max(valid ? best.kd : -INFINITY, s_r2);
  };

  // the neighbours in Morton order first: they shrink R2 the most
  for (int o = 1; o <= kNear; ++o) {
    if (b - o >= 0) visit(b - o);
    if (b + o < nb) visit(b + o);
  }
  // Every other box: a wave tests 64 AABBs at a time, a lane one of them,
  // against the query box's AABB, and then against the queries one by one (as
  // they stood at the start of the round: a k-th best only shrinks) until one
  // of them needs it, and ballots the survivors.  A box no query needs is then
  // never staged: a query box that holds one far point next to a dense part
  // of the cloud would otherwise stage all of that part, one box after the
  // other, each a load and two barriers.
  if (b - kNear > 0 || b + kNear < nb - 1) {
    for (int base = 0; base < nb; base += kBlock) {
      s_q[t] = make_float4(q.x, q.y, q.z, valid ? best.kd : -INFINITY);
      __syncthreads();
      const int box = base + t;
      bool keep = false;
      if (box < nb && (box < b - kNear || box > b + kNear)) {
        const float4 lo = box_lo[box], hi = box_hi[box];
        if (!(box_box_bound(lo_q, hi_q, lo, hi) > R2)) {
          for (int c = 0; c < own && !keep; ++c) {
            const float4 qq = s_q[c];
            keep = !(point_box_bound(qq, lo, hi) > qq.w);
          }
        }
      }
      const unsigned long long m = __ballot(keep);
      if ((t & 63) == 0) s_mask[t >> 6] = m;
      __syncthreads();
#pragma unroll 1
      for (int w = 0; w < kBlock / kWave; ++w) {
        const unsigned long long mw = s_mask[w];
        uint32_t m_lo = __builtin_amdgcn_readfirstlane((uint32_t)mw);
        uint32_t m_hi = __builtin_amdgcn_readfirstlane((uint32_t)(mw >> 32));
        while (m_lo) {
          const int bit = __ffs(m_lo) - 1;
          m_lo &= m_lo - 1;
          visit(base + w * kWave + bit);
        }
        while (m_hi) {
          const int bit = __ffs(m_hi) - 1;
          m_hi &= m_hi - 1;
          visit(base + w * kWave + 32 + bit);
        }
      }
      __syncthreads();
    }
  }

  if (!valid) return;
  const size_t row = (size_t)__float_as_uint(q.w);
  const int found = min(k, n - 1);
  if (a.dist2 || a.index) {
#pragma unroll
    for (int s = 0; s < K; ++s) {
      if (s < k) {
        if (a.dist2) a.dist2[row * (size_t)k + s] = best.d[s];
        if (a.index) a.index[row * (size_t)k + s] = best.j[s] == kNoRow ? -1 : best.j[s];
      }
    }
  }
  if (a.mean_dist2) {
    float sum = 0.f;  // ascending, in fp32
#pragma unroll
    for (int s = 0; s < K; ++s) {
      if (s < found) sum += best.d[s];
    }
    a.mean_dist2[row] = found > 0 ? sum / (float)found : 0.f;
  }
}

// ---------------------------------------------------------- workspace ----
constexpr int kMortonBits = 30;  // of each of the key's two words

struct Layout {
  size_t keys, vals, keys_alt, vals_alt, keys_hi, sort_ws, sort_ws_bytes, sorted, box_lo, box_hi, part, bbox, total;
};
inline size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
Layout layout_of(int32_t n) {
  Layout l;
  const size_t nb = div_up(n, kBox), words = up256(sizeof(uint32_t) * (size_t)n);
  size_t at = 0;
  l.keys = at, at += words;
  l.vals = at, at += words;
  l.keys_alt = at, at += words;
  l.vals_alt = at, at += words;
  l.keys_hi = at, at += words;
  l.sort_ws_bytes = gs_radix_sort_workspace_bytes(n);
  l.sort_ws = at, at += up256(l.sort_ws_bytes);
  l.sorted = at, at += up256(sizeof(float4) * (size_t)n);
  l.box_lo = at, at += up256(sizeof(float4) * nb);
  l.box_hi = at, at += up256(sizeof(float4) * nb);
  l.part = at, at += up256(2 * sizeof(float4) * nb);
  l.bbox = at, at += 256;
  l.total = at;
  return l;
}

}  // namespace

extern "C" size_t gs_knn_workspace_bytes(int32_t n) {
  if (n <= 0 || n > kMaxPoints) return 0;
  return layout_of(n).total;
}

extern "C" gs_status gs_knn(const gs_knn_args *a, gs_stream_t stream) {
  static const char *what = "gs_knn";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (a->k < 1 || a->k > GS_KNN_MAX_K) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: k must be in [1, 16]", what);
  if (a->n < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative n", what);
  if (a->n > kMaxPoints)
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: at most 2^30 (1073741824) points", what);
  if (!a->dist2 && !a->index && !a->mean_dist2)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null dist2, index and mean_dist2: nothing to write", what);
  if (a->n == 0) return GS_OK;
  if (!a->points) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null points", what);
  const Layout l = layout_of(a->n);
  if (!a->workspace || a->workspace_bytes < l.total || ((uintptr_t)a->workspace & 15u))
    return gs_internal_fail(GS_ERR_INVALID_ARG,
                            "%s: null, misaligned (16 B) or too small workspace (gs_knn_workspace_bytes)", what);
  hipStream_t s = (hipStream_t)stream;
  char *ws = (char *)a->workspace;
  const int n = a->n, nb = (int)div_up(n, kBox);
  uint32_t *keys = (uint32_t *)(ws + l.keys), *vals = (uint32_t *)(ws + l.vals);
  uint32_t *keys_alt = (uint32_t *)(ws + l.keys_alt), *vals_alt = (uint32_t *)(ws + l.vals_alt);
  uint32_t *keys_hi = (uint32_t *)(ws + l.keys_hi);
  float4 *sorted = (float4 *)(ws + l.sorted), *box_lo = (float4 *)(ws + l.box_lo), *box_hi = (float4 *)(ws + l.box_hi);
  float4 *part = (float4 *)(ws + l.part), *bbox = (float4 *)(ws + l.bbox);

  k_knn_bbox_blocks<<<nb, kBlock, 0, s>>>(a->points, n, part);
  k_knn_bbox_final<<<1, kBlock, 0, s>>>(part, nb, bbox);
  k_knn_morton<<<nb, kBlock, 0, s>>>(a->points, n, bbox, keys, keys_hi);
  if (gs_status st = gs_internal_check_launch(what)) return st;
  // two stable sorts of 30 bits: by the low word (values: the rows), then by the high word
  int32_t in_alt = 0;
  if (gs_status st = gs_internal_radix_sort_pairs(keys, vals, keys_alt, vals_alt, n, 0, kMortonBits, 1, ws + l.sort_ws,
                                                  l.sort_ws_bytes, &in_alt, nullptr, stream))
    return st;
  if (in_alt) {
    uint32_t *tk = keys, *tv = vals;
    keys = keys_alt, vals = vals_alt, keys_alt = tk, vals_alt = tv;
  }
  k_knn_high_keys<<<nb, kBlock, 0, s>>>(keys_hi, vals, n, keys);
  if (gs_status st = gs_internal_radix_sort_pairs(keys, vals, keys_alt, vals_alt, n, 0, kMortonBits, 0, ws + l.sort_ws,
                                                  l.sort_ws_bytes, &in_alt, nullptr, stream))
    return st;
  k_knn_gather<<<nb, kBlock, 0, s>>>(a->points, n, in_alt ? vals_alt : vals, sorted, box_lo, box_hi);
  if (a->k <= 4)
    k_knn_search<4><<<nb, kBlock, 0, s>>>(*a, sorted, box_lo, box_hi, nb);
  else if (a->k <= 8)
    k_knn_search<8><<<nb, kBlock, 0, s>>>(*a, sorted, box_lo, box_hi, nb);
  else
    k_knn_search<16><<<nb, kBlock, 0, s>>>(*a, sorted, box_lo, box_hi, nb);
  return gs_internal_check_launch(what);
}
