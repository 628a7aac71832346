// gs_bin.hip -- tile binning and the per-tile list ranges of the render path:
//   k_bin_*           renderer.py:263-298   tile binning, emitted in depth order
//   k_tile_ranges(4)  renderer.py:266       per-tile list ranges
// (src/core/renderer.py of the reference.)
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsplat_mi355x.h"
#include "gs_internal.h"
#include "gs_device.h"

namespace {

#ifndef GS_RANGES_X4
#define GS_RANGES_X4 1
#endif
constexpr int kBinChunk = kBlock * 4;            // 1024 Gaussians per binning block (2 and 1 rounds: slower)

// ======================================================== binning =========
// The binning workspace: 5 nb words of per-block partials, then the
// depth-ordered rectangles (n uint2, 16-B aligned).
__device__ __forceinline__ uint2 *sorted_rects(uint32_t *partials, int nb) {
  return reinterpret_cast<uint2 *>(partials + ((5 * nb + 3) & ~3));
}

// partials[0..nb): touches per block (depth order), partials[nb..2nb): visible per index chunk,
// [2nb..3nb): index-order slots per chunk, [3nb..5nb): depth-bits min / max per chunk
__global__ __launch_bounds__(kBlock) void k_bin_partials(gs_bin_args a, uint32_t *partials, int nb) {
  __shared__ uint32_t s_tmp3[3][kBlock / kWave];
  const long long base = (long long)blockIdx.x * kBinChunk;
  constexpr int kR = kBinChunk / kBlock;
  // Loads unconditional (clamped index) and all rounds' at once: two round
  // trips (ids, then their rects/vis) instead of two per round -- a load
  // under a branch is waited for at the branch's join.  The index-order
  // rects of the second half are requested here too.
  uint32_t gi[kR];
  uint2 rc_own[kR];
#pragma unroll
  for (int i = 0; i < kR; ++i) {
    const long long k = base + i * kBlock + threadIdx.x;
    const long long kc = k < a.n ? k : a.n - 1;
    gi[i] = a.sorted_ids[kc];
    rc_own[i] = reinterpret_cast<const uint2 *>(a.rects)[kc];
  }
  uint32_t sum = 0, nvis = 0;
  uint2 rc_d[kR];
  uint32_t vis_o[kR];
#pragma unroll
  for (int i = 0; i < kR; ++i) {
    const long long k = base + i * kBlock + threadIdx.x;
    rc_d[i] = reinterpret_cast<const uint2 *>(a.rects)[gi[i]];
    vis_o[i] = a.vis[k < a.n ? k : a.n - 1];  // M is a total: counted in index order (coalesced)
  }
#pragma unroll
  for (int i = 0; i < kR; ++i) {
    const long long k = base + i * kBlock + threadIdx.x;
    if (k < a.n) {
      sum += rect_touches(rc_d[i]);
      nvis += vis_o[i] ? 1u : 0u;
    }
  }
  // Gradient slots are numbered in Gaussian-index order (a Gaussian's
  // touches consecutive), so that gs_project_backward's threads g, g+1 read
  // adjacent slot ranges: here each Gaussian's exclusive prefix of touches
  // inside this block's index chunk (k_bin_emit adds the chunk's offset).
  uint32_t cnt[kR];
#pragma unroll
  for (int i = 0; i < kR; ++i) {
    const long long g = base + i * kBlock + threadIdx.x;
    cnt[i] = g < a.n ? rect_touches(rc_own[i]) : 0u;
  }
  // the block's touches (depth order) and visible count, and round 0's slot
  // prefix, in one scan
  uint3 t3;
  const uint3 e3 = block_exscan3(make_uint3(sum, nvis, cnt[0]), s_tmp3, &t3);
  if (threadIdx.x == 0) {
    partials[blockIdx.x] = t3.x;
    partials[nb + blockIdx.x] = t3.y;
  }
  // the depth-ordered rectangles, for k_bin_emit to read coalesced
  uint2 *srect = sorted_rects(partials, nb);
#pragma unroll
  for (int i = 0; i < kR; ++i) {
    const long long k = base + i * kBlock + threadIdx.x;
    if (k < a.n) srect[k] = rc_d[i];
  }
  // rounds 1..3's prefixes in one more scan (integer sums: any grouping)
  static_assert(kR == 4, "the slot prefix scans assume four rounds per binning block");
  uint3 u3;
  const uint3 f3 = block_exscan3(make_uint3(cnt[1], cnt[2], cnt[3]), s_tmp3, &u3);
  const uint32_t ex[kR] = {e3.z, f3.x, f3.y, f3.z};
  const uint32_t tt[kR] = {t3.z, u3.x, u3.y, u3.z};
  uint32_t carry = 0;
#pragma unroll
  for (int i = 0; i < kR; ++i) {
    const long long g = base + i * kBlock + threadIdx.x;
    if (g < a.n) a.pair_offset[g] = carry + ex[i];
    carry += tt[i];
  }
  if (threadIdx.x == 0) partials[2 * nb + blockIdx.x] = carry;
  // the projection blocks of this chunk (kBinChunk / kBlock of them): their
  // depth-bits min / max, folded for k_bin_scan_partials
  constexpr int kPB = kBinChunk / kBlock;
  if (threadIdx.x < kPB) {
    const int pb = blockIdx.x * kPB + threadIdx.x, npb = (a.n + kBlock - 1) / kBlock;
    const bool ok = pb < npb;
    uint32_t mn = ok ? a.key_minmax[2 * pb] : 0xFFFFFFFFu, mx = ok ? a.key_minmax[2 * pb + 1] : 0u;
#pragma unroll
    for (int d = 1; d < kPB; d <<= 1) {
      mn = min(mn, (uint32_t)__shfl_xor((int)mn, d, 64));
      mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
    }
    if (threadIdx.x == 0) {
      partials[3 * nb + blockIdx.x] = mn;
      partials[4 * nb + blockIdx.x] = mx;
    }
  }
}

// exclusive scan of the touch partials (single block); counters[0] = M, [1] = T,
// [2] / [3] = min / max visible depth bits (the projection's per-block values)
// The depth-key window held (rasterizer.window_holds): every visible bits(Z)
// - key_base below the window's limit -- 2^key_bits - 1, and 255 <<
// (key_bits - 8) from 9 bits on (gs_depth_sort_msd's sentinel bucket).
__device__ __forceinline__ bool window_held(uint32_t key_base, int key_bits, uint32_t zmin, uint32_t zmax) {
  if (key_bits <= 0 || key_bits >= 32 || zmin > zmax) return true;
  const uint64_t full = (1ull << key_bits) - 1ull;
  const uint64_t lim = key_bits >= 9 ? min(full, 255ull << (key_bits - 8)) : full;
  return zmin >= key_base && (uint64_t)(zmax - key_base) < lim;
}

__global__ __launch_bounds__(kBlock) void k_bin_scan_partials(gs_bin_args a, uint32_t *partials, int nb) {
  uint32_t *const counters = a.counters, *const host_counters = a.host_counters;
  __shared__ uint32_t s_tmp3[3][kBlock / kWave];
  __shared__ uint32_t s_mm[2][kBlock / kWave];
  uint32_t mn = 0xFFFFFFFFu, mx = 0u;
  uint32_t carry = 0, vis = 0, slots = 0;
  // a chunk's three partials loaded unconditionally (clamped index) and the
  // next chunk's in flight during this one's scans: no load waits under a
  // branch (the compiler waited for each conditional load at its join)
  auto ld = [&](int i, uint32_t *v) {
    const int ci = i < nb ? i : nb - 1;
    v[0] = partials[ci];
    v[1] = partials[nb + ci];
    v[2] = partials[2 * nb + ci];
    v[3] = partials[3 * nb + ci];
    v[4] = partials[4 * nb + ci];
  };
  uint32_t vn[5];
  ld((int)threadIdx.x, vn);
  for (int c = 0; c < nb; c += kBlock) {
    const int i = c + threadIdx.x;
    const uint32_t v0 = i < nb ? vn[0] : 0u, v1 = i < nb ? vn[1] : 0u, v2 = i < nb ? vn[2] : 0u;
    // (a clamped reload of the last chunk only repeats a value: harmless for min / max)
    mn = min(mn, vn[3]);
    mx = max(mx, vn[4]);
    ld(i + kBlock, vn);
    // touches (depth order), visible, index-order slot chunks (k_bin_partials):
    // exclusive offsets of the first and third in place
    uint3 t3;
    const uint3 e = block_exscan3(make_uint3(v0, v1, v2), s_tmp3, &t3);
    if (i < nb) {
      partials[i] = carry + e.x;
      partials[2 * nb + i] = slots + e.z;
    }
    carry += t3.x;
    vis += t3.y;
    slots += t3.z;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) {
    mn = min(mn, (uint32_t)__shfl_xor((int)mn, d, 64));
    mx = max(mx, (uint32_t)__shfl_xor((int)mx, d, 64));
  }
  if ((threadIdx.x & (kWave - 1)) == 0) {
    s_mm[0][threadIdx.x >> 6] = mn;
    s_mm[1][threadIdx.x >> 6] = mx;
  }
  __syncthreads();  // s_mm
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 0; w < kBlock / kWave; ++w) {
      mn = min(mn, s_mm[0][w]);
      mx = max(mx, s_mm[1][w]);
    }
    // what a device-resident frame cannot do on the device (GS_FRAME_*): its
    // later stages see T_eff = 0 entries (empty lists, memory-safe)
    uint32_t status = 0u;
    if ((long long)carry > a.capacity) status |= GS_FRAME_NEED_CAPACITY;
    if (!window_held(a.key_base, a.key_bits, mn, mx)) status |= GS_FRAME_WINDOW_MISS;
    if (vis == 0u) status |= GS_FRAME_EMPTY;
    counters[0] = vis;
    counters[1] = carry;
    counters[2] = mn;
    counters[3] = mx;
    counters[4] = status;
    counters[5] = status ? 0u : carry;
    uint32_t seq = a.host_seq;
    if (a.frame_seq) {  // (one block, one thread: a plain increment)
      seq = *a.frame_seq + 1u;
      *a.frame_seq = seq;
    }
    // the sticky step flags: the first frame that sets them is recorded for
    // the host (its replays from there on updated nothing)
    uint32_t sticky = status;
    bool first_fail = status != 0u;
    if (a.step_flags) {
      const uint32_t old = atomicOr(a.step_flags, status);
      sticky = old | status;
      first_fail = old == 0u && status != 0u;
    }
    if (host_counters) {  // (M, T, depth range, status) straight to the host's pinned buffer
      host_counters[0] = vis;
      host_counters[1] = carry;
      host_counters[2] = mn;
      host_counters[3] = mx;
      host_counters[5] = status;
      host_counters[6] = sticky;
      if (first_fail) host_counters[7] = seq;
      __threadfence_system();  // the counters reach the host before the sequence word
      host_counters[4] = seq;
      __threadfence_system();
    }
  }
}

// Emission, coalesced: per round of 256 depth-ordered Gaussians, scan their
// touch counts into LDS and mark each output position with its Gaussian (a
// byte per position, a window of kOwnerCap positions at a time: one window
// per round unless the round's rectangles average more than 64 tiles); then
// every thread writes consecutive output entries, looking its Gaussian up in
// one LDS read (a binary search over the offsets took 8 dependent ones).
// Runs [lo, hi) longer than kWaveFillRun, flagged per lane by `wide`, are
// written by the wave's active lanes together, one run after another:
// fill(position, value of the lane that owns the run).  Every active lane of
// the wave must call it (ballots and shuffles inside, outside the divergent
// fill loop); lanes with nothing to fill pass wide = false.  Lanes that have
// already left the kernel (a partial last wave) take no part: the stride is
// the number of active lanes, not 64.
constexpr uint32_t kWaveFillRun = 32;
template <typename Fill>
__device__ __forceinline__ void wave_fill_runs(bool wide, uint32_t lo, uint32_t hi, uint32_t value, Fill fill) {
  unsigned long long m = __ballot(wide);
  if (!m) return;
  const unsigned long long act = __ballot(1);
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t nact = (uint32_t)__popcll(act), rank = (uint32_t)__popcll(act & ((1ull << lane) - 1ull));
  while (m) {
    const int l = __ffsll(m) - 1;
    m &= m - 1;
    const uint32_t rlo = (uint32_t)__shfl((int)lo, l, 64), rhi = (uint32_t)__shfl((int)hi, l, 64);
    const uint32_t v = (uint32_t)__shfl((int)value, l, 64);
    for (uint32_t o = rlo + rank; o < rhi; o += nact) fill(o, v);
  }
}

constexpr uint32_t kOwnerCap = kBlock * 64;
__global__ __launch_bounds__(kBlock) void k_bin_emit(gs_bin_args a, const uint32_t *partials) {
  __shared__ uint32_t s_off[kBlock + 1];
  __shared__ uint32_t s_g[kBlock];
  __shared__ uint2 s_rect[kBlock];
  __shared__ uint32_t s_tmp[4];
  __shared__ uint32_t s_tmp3[3][kBlock / kWave];
  __shared__ uint8_t s_owner[kOwnerCap];
  const long long base = (long long)blockIdx.x * kBinChunk;
  // a device-resident frame that failed (gs_bin_count's status): no entry is
  // emitted and every rectangle of the chunk is cleared, so the frame's
  // backward gathers zero slots per Gaussian -- never a slot past the
  // capacity (the caller redoes the frame on the host path)
  if (a.device_counts && a.counters[4] != 0u) {
    for (int r = 0; r < kBinChunk / kBlock; ++r) {
      const long long g = base + r * kBlock + threadIdx.x;
      if (g < a.n) reinterpret_cast<uint2 *>(const_cast<uint32_t *>(a.rects))[g] = make_uint2(1u, 1u);
    }
    return;
  }
  // T entries do not fit: do nothing (the caller re-emits into T-sized
  // buffers; the slot pass below is not idempotent, so it must run once)
  const uint32_t T = a.counters[1];
  if ((long long)T > a.capacity) return;
  uint32_t out_base = partials[blockIdx.x];
  constexpr int kR = kBinChunk / kBlock;
  // all rounds' ids and rects unconditionally (clamped): one round trip for
  // the block
  uint32_t gr[kR];
  uint2 rcr[kR];
  uint32_t offr[kR];
  const uint2 *srect = sorted_rects(const_cast<uint32_t *>(partials), (int)gridDim.x);
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const long long k = base + r * kBlock + threadIdx.x;
    const long long kc = k < a.n ? k : a.n - 1;
    gr[r] = a.sorted_ids[kc];
    rcr[r] = srect[kc];  // (k_bin_partials' depth-ordered copy: no gather by id)
    offr[r] = a.pair_offset[kc];  // (index order, for the slot pass below)
  }
  // every round's touch counts and their prefixes up front (three rounds in
  // one scan: the scans are latency-bound)
  static_assert(kR == 4, "the emission's prefix scans assume four rounds per binning block");
  uint32_t cntr[kR];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const long long k = base + r * kBlock + threadIdx.x;
    if (k < a.n) {
      cntr[r] = rect_touches(rcr[r]);
    } else {
      cntr[r] = 0u;
      gr[r] = 0xFFFFFFFFu;
      rcr[r] = make_uint2(1u, 1u);
    }
  }
  uint3 ta;
  uint32_t tb;
  const uint3 ea = block_exscan3(make_uint3(cntr[0], cntr[1], cntr[2]), s_tmp3, &ta);
  const uint32_t eb = block_exscan(cntr[3], s_tmp, &tb);
  const uint32_t exr[kR] = {ea.x, ea.y, ea.z, eb}, totr[kR] = {ta.x, ta.y, ta.z, tb};
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const uint32_t g = gr[r], cnt = cntr[r], ex = exr[r], tot = totr[r];
    const uint2 rc = rcr[r];
    if (r) __syncthreads();  // the previous round's owner-map and offset reads are done
    s_off[threadIdx.x] = ex;
    s_g[threadIdx.x] = g;
    s_rect[threadIdx.x] = rc;
    if (threadIdx.x == 0) s_off[kBlock] = tot;
    // (tot is block-uniform: every thread runs the same windows)
    for (uint32_t wb = 0; wb < tot; wb += kOwnerCap) {
      if (wb) __syncthreads();  // the previous window's owner reads are done
      const uint32_t lo_c = ex > wb ? ex : wb, hi_c = min(ex + cnt, wb + kOwnerCap);
      // short runs by their own lane; a wide rectangle's run (up to a whole
      // window) by its wave, 64 entries per step
      const bool wide = hi_c > lo_c + kWaveFillRun;
      if (!wide)
        for (uint32_t o = lo_c; o < hi_c; ++o) s_owner[o - wb] = (uint8_t)threadIdx.x;
      wave_fill_runs(wide, lo_c - wb, hi_c - wb, threadIdx.x, [&](uint32_t o, uint32_t owner) {
        s_owner[o] = (uint8_t)owner;
      });
      __syncthreads();
      const uint32_t wend = min(tot, wb + kOwnerCap);
      for (uint32_t o = wb + threadIdx.x; o < wend; o += kBlock) {
        const int lo = s_owner[o - wb];
        const uint2 rr = s_rect[lo];
        const uint32_t tx0 = rr.x & 0xFFFFu, ty0 = rr.y & 0xFFFFu;
        const uint32_t wt = (rr.x >> 16) - tx0 + 1u;
        const uint32_t loc = o - s_off[lo];
        const uint32_t row = loc / wt;
        const uint32_t key = (ty0 + row) * (uint32_t)a.tiles_x + tx0 + (loc - row * wt);
        a.tile_keys[out_base + o] = key;
        a.pair_gauss[out_base + o] = s_g[lo];
      }
    }
    out_base += tot;
  }
  // Gradient slots, in Gaussian-index order over this block's index chunk
  // (coalesced): the chunk's offset + each Gaussian's prefix in the chunk
  // (k_bin_partials); the first slot is also kept in the record (word 10) for
  // the backward.  Records of culled Gaussians are never read.
  const uint32_t cbase = partials[2 * gridDim.x + blockIdx.x];
#pragma unroll
  for (int r = 0; r < kR; ++r) {
    const long long g = base + r * kBlock + threadIdx.x;
    if (g < a.n) {
      const uint32_t slot = cbase + offr[r];
      a.pair_offset[g] = slot;
      a.records[(size_t)g * GS_RECORD_FLOATS + 10] = __uint_as_float(slot);
    }
  }
}

// A failed device-resident frame's pixels (gs_bin_count's status non-zero):
// what a frame that draws nothing shows (renderer.py:74-83) -- the background
// once, zero alpha and depth -- over the empty-list blend's bg + 1 * bg.  A
// frame that succeeded leaves after one scalar load per wave.  Grid-stride.
__global__ __launch_bounds__(kBlock) void k_failed_frame_pixels(const uint32_t *counters, float *image, float *alpha,
                                                               float *depth, long long HW, float bg0, float bg1,
                                                               float bg2) {
  if (counters[4] == 0u) return;
  for (long long p = (long long)blockIdx.x * kBlock + threadIdx.x; p < HW; p += (long long)gridDim.x * kBlock) {
    image[p] = bg0;
    image[HW + p] = bg1;
    image[2 * HW + p] = bg2;
    alpha[p] = 0.f;
    depth[p] = 0.f;
  }
}

// Every tile's [start, end) from the tile-sorted keys, empty tiles included
// (no memset): position p in [0, T] is a boundary when key[p-1] != key[p]
// (key[-1] = -1, key[T] = num_tiles); it closes the previous tile, opens the
// next and writes the tiles in between as empty at p.
// Four consecutive positions per thread (the default tile's four-cell slot
// flags): one 16-B key load, the previous key from the neighbouring lane, one
// 16-B flag store.  Same writes as k_tile_ranges.
__global__ __launch_bounds__(kBlock) void k_tile_ranges4(gs_range_args a) {
  const long long p0 = 4 * ((long long)blockIdx.x * kBlock + threadIdx.x);
  const long long T = live_items(a.num_pairs, a.num_pairs_dev);
  if (p0 > T) return;
  const int lane = threadIdx.x & 63;
  uint4 k = make_uint4(0u, 0u, 0u, 0u);
  if (p0 + 3 < T) {
    k = reinterpret_cast<const uint4 *>(a.sorted_keys)[p0 / 4];
  } else {
    if (p0 < T) k.x = a.sorted_keys[p0];
    if (p0 + 1 < T) k.y = a.sorted_keys[p0 + 1];
    if (p0 + 2 < T) k.z = a.sorted_keys[p0 + 2];
  }
  // the key before p0: the previous lane's last one (its positions end at p0 - 1)
  uint32_t before = (uint32_t)__shfl_up((int)k.w, 1, 64);
  if (lane == 0) before = p0 > 0 ? a.sorted_keys[p0 - 1] : 0u;
  if (a.slot_live) {
    if (p0 + 3 < T)
      reinterpret_cast<uint4 *>(a.slot_live)[p0 / 4] = make_uint4(0u, 0u, 0u, 0u);
    else
      for (long long q = p0; q < T; ++q) reinterpret_cast<uint32_t *>(a.slot_live)[q] = 0u;
  }
  const uint32_t kk[4] = {k.x, k.y, k.z, k.w};
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const long long p = p0 + i;
    const bool in = p <= T;  // (lanes past the end take part in the wave fills with nothing to fill)
    const long long prev = !in ? 0 : (p > 0 ? (long long)(i ? kk[i - 1] : before) : -1);
    const long long cur = !in ? 0 : (p < T ? (long long)kk[i] : (long long)a.num_tiles);
    const bool edge = in && cur != prev;
    if (edge && prev >= 0) a.ranges[2 * prev + 1] = (uint32_t)p;
    if (edge && cur < a.num_tiles) a.ranges[2 * cur] = (uint32_t)p;
    const uint32_t t0 = (uint32_t)(prev + 1), t1 = edge ? (uint32_t)cur : t0;
    const bool wide = edge && t1 > t0 + kWaveFillRun;
    if (edge && !wide)
      for (uint32_t t = t0; t < t1; ++t) a.ranges[2 * t] = a.ranges[2 * t + 1] = (uint32_t)p;
    wave_fill_runs(wide, t0, t1, (uint32_t)p, [&](uint32_t t, uint32_t q) { a.ranges[2 * t] = a.ranges[2 * t + 1] = q; });
  }
}

__global__ __launch_bounds__(kBlock) void k_tile_ranges(gs_range_args a) {
  const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
  a.num_pairs = live_items(a.num_pairs, a.num_pairs_dev);
  if (p > a.num_pairs) return;
  if (a.slot_live && p < a.num_pairs) {  // slot p's flags for the backward (coalesced)
    if (a.cells == 4)
      reinterpret_cast<uint32_t *>(a.slot_live)[p] = 0u;
    else if (a.cells == 1)
      a.slot_live[p] = 0;
    else
      for (int c = 0; c < a.cells; ++c) a.slot_live[p * a.cells + c] = 0;
  }
  const long long prev = p > 0 ? (long long)a.sorted_keys[p - 1] : -1;
  const long long cur = p < a.num_pairs ? (long long)a.sorted_keys[p] : (long long)a.num_tiles;
  const bool edge = cur != prev;
  if (edge && prev >= 0) a.ranges[2 * prev + 1] = (uint32_t)p;
  if (edge && cur < a.num_tiles) a.ranges[2 * cur] = (uint32_t)p;
  // the empty tiles in between: a short gap by its lane, a long one (a sparse
  // frame) by the wave, 64 tiles per step
  const uint32_t t0 = (uint32_t)(prev + 1), t1 = edge ? (uint32_t)cur : t0;
  const bool wide = t1 > t0 + kWaveFillRun;
  if (!wide)
    for (uint32_t t = t0; t < t1; ++t) a.ranges[2 * t] = a.ranges[2 * t + 1] = (uint32_t)p;
  wave_fill_runs(wide, t0, t1, (uint32_t)p, [&](uint32_t t, uint32_t q) { a.ranges[2 * t] = a.ranges[2 * t + 1] = q; });
}

}  // namespace

// ============================================================ C ABI =======
extern "C" {

size_t gs_bin_workspace_bytes(int32_t n) {
  const size_t nb = n > 0 ? div_up(n, kBinChunk) : 1;
  return sizeof(uint32_t) * ((5 * nb + 3) & ~(size_t)3) + sizeof(uint32_t) * 2 * (size_t)(n > 0 ? n : 0) + 256;
}

gs_status gs_bin_count(const gs_bin_args *a, gs_stream_t stream) {
  if (!a || !a->counters) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", "gs_bin_count");
  if (a->n <= 0) return GS_OK;
  if (!a->sorted_ids || !a->rects || !a->vis || !a->pair_offset || !a->workspace || !a->key_minmax ||
      a->workspace_bytes < gs_bin_workspace_bytes(a->n))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer or workspace too small", "gs_bin_count");
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)div_up(a->n, kBinChunk);
  uint32_t *partials = (uint32_t *)a->workspace;
  k_bin_partials<<<nb, kBlock, 0, s>>>(*a, partials, nb);
  k_bin_scan_partials<<<1, kBlock, 0, s>>>(*a, partials, nb);
  return gs_internal_check_launch("gs_bin_count");
}

gs_status gs_bin_emit(const gs_bin_args *a, gs_stream_t stream) {
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", "gs_bin_emit");
  if (a->n <= 0) return GS_OK;
  if (!a->sorted_ids || !a->rects || !a->counters || !a->workspace || !a->tile_keys || !a->pair_gauss ||
      !a->pair_offset || !a->records)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", "gs_bin_emit");
  if (a->workspace_bytes < gs_bin_workspace_bytes(a->n))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: workspace too small", "gs_bin_emit");
  if (a->capacity < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative capacity", "gs_bin_emit");
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)div_up(a->n, kBinChunk);
  k_bin_emit<<<nb, kBlock, 0, s>>>(*a, (const uint32_t *)a->workspace);
  return gs_internal_check_launch("gs_bin_emit");
}

gs_status gs_tile_ranges(const gs_range_args *a, gs_stream_t stream) {
  if (!a || !a->ranges) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", "gs_tile_ranges");
  hipStream_t s = (hipStream_t)stream;
  if (a->num_pairs < 0 || a->num_tiles < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative size", "gs_tile_ranges");
  if (a->num_tiles == 0) return GS_OK;
  if (a->num_pairs > 0 && !a->sorted_keys) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", "gs_tile_ranges");
  if (a->slot_live && (a->cells < 1 || (a->cells == 4 && (reinterpret_cast<uintptr_t>(a->slot_live) & 3u))))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: slot_live needs cells >= 1 (4-B aligned at 4 cells)", "gs_tile_ranges");
  // four positions per thread where the flags are 4-B words (the default
  // tile) and the keys 16-B aligned
  if (GS_RANGES_X4 && (!a->slot_live || a->cells == 4) && (reinterpret_cast<uintptr_t>(a->sorted_keys) & 15u) == 0 &&
      (reinterpret_cast<uintptr_t>(a->slot_live) & 15u) == 0)
    k_tile_ranges4<<<div_up(a->num_pairs / 4 + 1, kBlock), kBlock, 0, s>>>(*a);
  else
    k_tile_ranges<<<div_up(a->num_pairs + 1, kBlock), kBlock, 0, s>>>(*a);
  return gs_internal_check_launch("gs_tile_ranges");
}

}  // extern "C"

gs_status gs_internal_failed_frame_pixels(const uint32_t *counters, const gs_camera *cam, float *image, float *alpha,
                                          float *depth, gs_stream_t stream) {
  if (!counters || !cam || !image || !alpha || !depth)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", "gs_internal_failed_frame_pixels");
  const long long HW = (long long)cam->image_width * cam->image_height;
  if (HW <= 0) return GS_OK;
  const unsigned blocks = div_up(HW, kBlock);
  k_failed_frame_pixels<<<blocks < 256u ? blocks : 256u, kBlock, 0, (hipStream_t)stream>>>(
      counters, image, alpha, depth, HW, cam->bg[0], cam->bg[1], cam->bg[2]);
  return gs_internal_check_launch("gs_internal_failed_frame_pixels");
}
