// gs_sort.hip -- the sorts of the render path, replacing the reference's
// stable sorts (src/core/renderer.py:231-237: depth, then tile id):
//   k_radix_hist/scan/scatter   stable LSD radix sort, no global atomics
//   k_msd_bucket_sort           one MSD pass + per-bucket LDS sorts (depth keys),
//                               and the one-workgroup sort of a small array
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsplat_mi355x.h"
#include "gs_internal.h"
#include "gs_device.h"

namespace {

constexpr int kRadixBits = 8;
constexpr int kRadix = 1 << kRadixBits;
#ifndef GS_SORT_IPT
#define GS_SORT_IPT 8
#endif
constexpr int kSortIpt = GS_SORT_IPT;            // items per thread per sort block (4, 16: slower)
constexpr int kSortChunk = kBlock * kSortIpt;    // 2048 items per block

__device__ __forceinline__ uint32_t div_up_dev(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a + b - 1) / b); }

__device__ __forceinline__ unsigned long long lanemask_lt() {
  const int lane = threadIdx.x & (kWave - 1);
  return (lane == 0) ? 0ull : ((~0ull) >> (64 - lane));
}

// Lanes of the wave holding the same `nbits`-bit digit (match-any via ballots).
__device__ __forceinline__ unsigned long long match_digit(uint32_t d, int nbits, unsigned long long m) {
  for (int b = 0; b < nbits; ++b) {
    const bool bit = (d >> b) & 1u;
    const unsigned long long bb = __ballot(bit);
    m &= bit ? bb : ~bb;
  }
  return m;
}

// ===================================================== radix sort =========
// Pass p sorts digit (key >> shift) & mask.  One block = kSortChunk items;
// wave w owns the contiguous quarter of the chunk, walked in kSortIpt rounds
// of 64 (order = wave, round, lane: stable).  No global atomics: per-block
// digit counts -> per-digit row scan (+ row totals) -> the scatter derives
// the digit bases from the 256 totals itself.
// n_dev (a device-resident frame's tile sort, launched before T is known on
// the host): the items are min(*n_dev, n) (live_items); n -- the capacity -- sizes the
// grid and nb stays the count table's row stride.  Blocks past the items
// leave at once; the scans run over the live blocks' columns only.

__global__ __launch_bounds__(kBlock) void k_radix_hist(const uint32_t *__restrict__ keys, int n, int shift,
                                                       int nbits, uint32_t *counts, int nb,
                                                       const uint32_t *n_dev = nullptr) {
  n = live_items(n, n_dev);
  if ((long long)blockIdx.x * kSortChunk >= n) return;
  __shared__ uint32_t hist[kRadix];
  hist[threadIdx.x] = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t mask = (1u << nbits) - 1u;
  const long long base = (long long)blockIdx.x * kSortChunk + wave * (kSortChunk / 4);
  // all rounds' keys in one round trip: unconditional loads (clamped index;
  // a load under a branch is waited for at its join)
  uint32_t kr[kSortIpt];
#pragma unroll
  for (int r = 0; r < kSortIpt; ++r) {
    const long long idx = base + r * 64 + lane;
    kr[r] = keys[idx < n ? idx : n - 1];
  }
  // one LDS atomic per key (the LDS serialises equal addresses itself;
  // ballot-matched digit counts were 9 us slower on the tile sort)
#pragma unroll
  for (int r = 0; r < kSortIpt; ++r) {
    const long long idx = base + r * 64 + lane;
    if (idx < n) atomicAdd(&hist[(kr[r] >> shift) & mask], 1u);
  }
  __syncthreads();
  if (threadIdx.x <= mask) counts[(size_t)threadIdx.x * nb + blockIdx.x] = hist[threadIdx.x];
}

// row d of counts -> exclusive prefix over blocks; totals[d] = row sum.
// Thread t owns a contiguous run of `per` (<= kScanPer) entries of each
// 256 * per stretch (loads all in flight): one block scan per stretch (nb <=
// 4096, 8.4M keys: one) instead of one per 256 entries.
constexpr int kScanPer = 16;
__global__ __launch_bounds__(kBlock) void k_radix_scan(uint32_t *counts, uint32_t *totals, int nb,
                                                       const uint32_t *n_dev = nullptr) {
  __shared__ uint32_t s_tmp[4];
  const int d = blockIdx.x;
  uint32_t *row = counts + (size_t)d * nb;  // (row stride: the launch's nb)
  if (n_dev) nb = min(nb, (int)div_up_dev(*n_dev, kSortChunk));
  const int per = min(kScanPer, (nb + kBlock - 1) / kBlock);
  uint32_t carry = 0, tot;
  for (int c = 0; c < nb; c += kBlock * per) {
    const int i0 = c + (int)threadIdx.x * per;
    uint32_t v[kScanPer];
    uint32_t sum = 0;
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
      v[k] = (k < per && i0 + k < nb) ? row[i0 + k] : 0u;
      sum += v[k];
    }
    uint32_t run = carry + block_exscan(sum, s_tmp, &tot);
#pragma unroll
    for (int k = 0; k < kScanPer; ++k) {
      if (k < per && i0 + k < nb) row[i0 + k] = run;
      run += v[k];
    }
    carry += tot;
  }
  if (threadIdx.x == 0) totals[d] = carry;
}

template <bool kIota>  // values = input positions (the first pass of an iota-valued sort)
__global__ __launch_bounds__(kBlock) void k_radix_scatter(const uint32_t *__restrict__ keys_in,
                                                          const uint32_t *__restrict__ vals_in,
                                                          uint32_t *__restrict__ keys_out,
                                                          uint32_t *__restrict__ vals_out, int n, int shift,
                                                          int nbits, const uint32_t *counts,
                                                          const uint32_t *totals, int nb,
                                                          const uint32_t *n_dev = nullptr) {
  n = live_items(n, n_dev);
  if ((long long)blockIdx.x * kSortChunk >= n) return;
  __shared__ uint32_t wcnt[4][kRadix];
  __shared__ uint32_t s_lbase[kRadix];  // block-local start of each digit
  __shared__ uint32_t s_gbase[kRadix];  // global start of this block's run of each digit
  __shared__ uint32_t s_k[kSortChunk], s_v[kSortChunk];
  __shared__ uint32_t s_tmp[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int w = 0; w < 4; ++w) wcnt[w][threadIdx.x] = 0;
  const uint32_t mask = (1u << nbits) - 1u;
  const long long blk0 = (long long)blockIdx.x * kSortChunk;
  const long long base = blk0 + wave * (kSortChunk / 4);
  // all rounds' keys and values in one round trip (unconditional, clamped),
  // requested before the digit-base scan so that they fly during it
  uint32_t k_[kSortIpt], v_[kSortIpt];
#pragma unroll
  for (int r = 0; r < kSortIpt; ++r) {
    const long long idx = base + r * 64 + lane;
    const long long ci = idx < n ? idx : n - 1;
    k_[r] = keys_in[ci];
    v_[r] = kIota ? (uint32_t)idx : vals_in[ci];
  }
  // (also in flight; rows and totals exist for the pass's 2^nbits digits only)
  const bool dig = threadIdx.x <= mask;
  const uint32_t my_prefix = dig ? counts[(size_t)threadIdx.x * nb + blockIdx.x] : 0u;
  uint32_t tot;
  const uint32_t dbase = block_exscan(dig ? totals[threadIdx.x] : 0u, s_tmp, &tot);  // includes a barrier
  uint32_t rk[kSortIpt];
#pragma unroll
  for (int r = 0; r < kSortIpt; ++r) {
    const long long idx = base + r * 64 + lane;
    const bool valid = idx < n;
    const uint32_t key = valid ? k_[r] : 0u;
    const uint32_t val = valid ? v_[r] : 0u;
    const uint32_t d = (key >> shift) & mask;
    const unsigned long long m = match_digit(d, nbits, __ballot(valid));
    const uint32_t below = (uint32_t)__popcll(m & lanemask_lt());
    uint32_t old = 0;
    if (valid) old = wcnt[wave][d];
    if (valid && below == 0) wcnt[wave][d] = old + (uint32_t)__popcll(m);
    k_[r] = key;
    v_[r] = val;
    rk[r] = valid ? old + below : 0xFFFFFFFFu;
  }
  __syncthreads();
  {
    // per digit: wave prefixes inside the block, block count, then the
    // block-local digit start (scan over digits)
    uint32_t run = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const uint32_t t = wcnt[w][threadIdx.x];
      wcnt[w][threadIdx.x] = run;
      run += t;
    }
    const uint32_t lb = block_exscan(run, s_tmp, &tot);  // barrier inside
    s_lbase[threadIdx.x] = lb;
    s_gbase[threadIdx.x] = dbase + my_prefix;
  }
  __syncthreads();
  // locally sorted chunk in LDS (stable: wave, round, lane order within a digit)
#pragma unroll
  for (int r = 0; r < kSortIpt; ++r) {
    if (rk[r] != 0xFFFFFFFFu) {
      const uint32_t d = (k_[r] >> shift) & mask;
      const uint32_t lp = s_lbase[d] + wcnt[wave][d] + rk[r];
      s_k[lp] = k_[r];
      s_v[lp] = v_[r];
    }
  }
  __syncthreads();
  // write out: consecutive threads -> consecutive positions of one digit run
  const int cnt = (int)min((long long)kSortChunk, (long long)n - blk0);
  for (int i = threadIdx.x; i < cnt; i += kBlock) {
    const uint32_t key = s_k[i];
    const uint32_t d = (key >> shift) & mask;
    const uint32_t dst = s_gbase[d] + (uint32_t)i - s_lbase[d];
    keys_out[dst] = key;
    vals_out[dst] = s_v[i];
  }
}

// Bucket sort after one MSD pass (gs_depth_sort_msd): workgroup d sorts the
// items whose top 8 key bits are d -- a contiguous, index-ordered run of the
// MSD pass's output -- by their low `lowbits` bits, in LDS, in place.  Stable
// LSD passes as in k_radix_scatter (wave w owns a contiguous segment, walked
// in rounds of 64; ballot match ranking), but the data stays in LDS between
// passes.  Bucket 255 holds the culled sentinel only (the caller's window
// keeps visible keys below 255 << lowbits) and is left as the MSD pass wrote
// it: index order, what the LSD sort gives equal keys.  A bucket over
// kMsdCap items is left unsorted and flagged: 0xFFFFFFFF in *overflow (the
// caller's depth-max word, so its window check fails and it sorts again).
constexpr int kMsdThreads = 1024;
constexpr int kMsdWaves = kMsdThreads / kWave;
constexpr int kMsdIpt = 16;
constexpr int kMsdCap = kMsdThreads * kMsdIpt;  // 16384 items: 128 KB of keys + values in LDS

// kWhole (gs_internal_small_sort): one workgroup sorts a whole array of
// n <= kMsdCap keys by their low `lowbits` bits -- the bucket is everything,
// read from keys / vals (vals NULL: the input positions) and written to
// keys_out / vals_out.  One launch instead of a radix sort's 3 per pass, for
// the small frames whose steps are bound by launches.
template <bool kWhole = false>
__global__ __launch_bounds__(kMsdThreads) void k_msd_bucket_sort(uint32_t *__restrict__ keys,
                                                               uint32_t *__restrict__ vals,
                                                               const uint32_t *__restrict__ totals, int lowbits,
                                                               uint32_t *overflow, uint32_t whole_n = 0u,
                                                               uint32_t *__restrict__ keys_out = nullptr,
                                                               uint32_t *__restrict__ vals_out = nullptr,
                                                               const uint32_t *whole_n_dev = nullptr) {
  if (kWhole && whole_n_dev) whole_n = min(whole_n, *whole_n_dev);  // (a device-resident frame's T)
  __shared__ uint32_t s_k[kMsdCap], s_v[kMsdCap];
  __shared__ uint32_t wcnt[kMsdWaves][kRadix];
  __shared__ uint32_t s_lbase[kRadix];
  __shared__ uint32_t s_tmp[4];
  __shared__ uint32_t s_seg[2];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const uint32_t d0 = blockIdx.x;  // the bucket (grid: 255; bucket 255 is never sorted)
  if (kWhole) {
    if (threadIdx.x == 0) {
      s_seg[0] = 0u;
      s_seg[1] = whole_n;
    }
  } else if (wave == 0) {
    // start = totals[0 .. d0) summed, size = totals[d0]
    uint32_t s = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const uint32_t t = (uint32_t)(4 * lane + k);
      s += t < d0 ? totals[t] : 0u;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) s += (uint32_t)__shfl_xor((int)s, o, 64);
    if (lane == 0) {
      s_seg[0] = s;
      s_seg[1] = totals[d0];
    }
  }
  __syncthreads();
  const uint32_t start = s_seg[0], size = s_seg[1];
  if constexpr (kWhole) {
    if (size <= 1u) {
      if (threadIdx.x == 0 && size == 1u) {
        keys_out[0] = keys[0];
        vals_out[0] = vals ? vals[0] : 0u;
      }
      return;
    }
  } else if (size <= 1u) {
    return;
  }
  if (size > (uint32_t)kMsdCap) {
    if (threadIdx.x == 0) *overflow = 0xFFFFFFFFu;
    return;
  }
  // wave w: items [w seg, (w + 1) seg), seg a multiple of 64; order (wave, round, lane)
  const uint32_t seg = (size + kMsdThreads - 1) / kMsdThreads * kWave;
  const int rounds = (int)(seg / kWave);
  // every round's key and value requested at once: unconditional loads of a
  // clamped index (a load under a branch is waited for at its join)
  uint32_t k_[kMsdIpt], v_[kMsdIpt];
#pragma unroll
  for (int r = 0; r < kMsdIpt; ++r) {
    const uint32_t i = (uint32_t)wave * seg + (uint32_t)(r * kWave + lane);
    const uint32_t ic = (r < rounds && i < size) ? i : 0u;
    k_[r] = keys[start + ic];
    v_[r] = (kWhole && !vals) ? ic : vals[start + ic];
  }
  const int passes = (lowbits + kRadixBits - 1) / kRadixBits;
  int shift = 0;
  for (int p = 0; p < passes; ++p) {
    const int nbits = (lowbits - shift + (passes - p) - 1) / (passes - p);
    const uint32_t mask = (1u << nbits) - 1u;
    for (int t = threadIdx.x; t < kMsdWaves * kRadix; t += kMsdThreads) (&wcnt[0][0])[t] = 0u;
    __syncthreads();
    uint32_t rk[kMsdIpt];
#pragma unroll
    for (int r = 0; r < kMsdIpt; ++r) {
      rk[r] = 0xFFFFFFFFu;
      if (r < rounds) {  // wave-uniform
        const uint32_t i = (uint32_t)wave * seg + (uint32_t)(r * kWave + lane);
        const bool valid = i < size;
        const uint32_t dg = (k_[r] >> shift) & mask;
        const unsigned long long m = match_digit(dg, nbits, __ballot(valid));
        const uint32_t below = (uint32_t)__popcll(m & lanemask_lt());
        uint32_t old = 0;
        if (valid) old = wcnt[wave][dg];
        if (valid && below == 0) wcnt[wave][dg] = old + (uint32_t)__popcll(m);
        if (valid) rk[r] = old + below;
      }
    }
    __syncthreads();
    // per digit: wave prefixes, then the block-local digit start (scan over
    // the 256 digits by the first four waves)
    uint32_t run = 0;
    if (threadIdx.x < kRadix) {
      for (int w = 0; w < kMsdWaves; ++w) {
        const uint32_t t = wcnt[w][threadIdx.x];
        wcnt[w][threadIdx.x] = run;
        run += t;
      }
    }
    uint32_t incl = run;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t t = (uint32_t)__shfl_up((int)incl, o, 64);
      if (lane >= o) incl += t;
    }
    if (threadIdx.x < kRadix && lane == 63) s_tmp[wave] = incl;
    __syncthreads();
    if (threadIdx.x < kRadix) {
      uint32_t base = 0;
      for (int w = 0; w < wave; ++w) base += s_tmp[w];
      s_lbase[threadIdx.x] = base + incl - run;
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < kMsdIpt; ++r) {
      if (rk[r] != 0xFFFFFFFFu) {
        const uint32_t dg = (k_[r] >> shift) & mask;
        const uint32_t lp = s_lbase[dg] + wcnt[wave][dg] + rk[r];
        s_k[lp] = k_[r];
        s_v[lp] = v_[r];
      }
    }
    __syncthreads();
    shift += nbits;
    if (p + 1 < passes) {
#pragma unroll
      for (int r = 0; r < kMsdIpt; ++r) {
        const uint32_t i = (uint32_t)wave * seg + (uint32_t)(r * kWave + lane);
        const uint32_t ic = (r < rounds && i < size) ? i : 0u;  // (unconditional, as above)
        k_[r] = s_k[ic];
        v_[r] = s_v[ic];
      }
    }
  }
  uint32_t *ko = kWhole ? keys_out : keys, *vo = kWhole ? vals_out : vals;
  for (uint32_t i = threadIdx.x; i < size; i += kMsdThreads) {
    ko[start + i] = s_k[i];
    vo[start + i] = s_v[i];
  }
}

}  // namespace

// ============================================================ C ABI =======
extern "C" {

size_t gs_radix_sort_workspace_bytes(int32_t n) {
  const size_t nb = n > 0 ? div_up(n, kSortChunk) : 1;
  return sizeof(uint32_t) * (kRadix * nb + kRadix) + 256;
}

gs_status gs_radix_sort_pairs(uint32_t *keys, uint32_t *vals, uint32_t *keys_alt, uint32_t *vals_alt,
                              int32_t n, int32_t begin_bit, int32_t end_bit, int32_t vals_are_iota,
                              void *workspace, size_t workspace_bytes, int32_t *result_in_alt,
                              gs_stream_t stream) {
  return gs_internal_radix_sort_pairs(keys, vals, keys_alt, vals_alt, n, begin_bit, end_bit, vals_are_iota,
                                      workspace, workspace_bytes, result_in_alt, nullptr, stream);
}

}  // extern "C"

gs_status gs_internal_radix_sort_pairs(uint32_t *keys, uint32_t *vals, uint32_t *keys_alt, uint32_t *vals_alt,
                                       int32_t n, int32_t begin_bit, int32_t end_bit, int32_t vals_are_iota,
                                       void *workspace, size_t workspace_bytes, int32_t *result_in_alt,
                                       const uint32_t *n_dev, gs_stream_t stream) {
  if (!result_in_alt) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null result_in_alt", "gs_radix_sort_pairs");
  if (begin_bit < 0 || end_bit > 32 || begin_bit >= end_bit || n < 0)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: bad bit range / n", "gs_radix_sort_pairs");
  const int passes = (end_bit - begin_bit + kRadixBits - 1) / kRadixBits;
  *result_in_alt = passes & 1;
  if (n == 0) return GS_OK;
  if (!keys || !vals || !keys_alt || !vals_alt || !workspace ||
      workspace_bytes < gs_radix_sort_workspace_bytes(n))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer or workspace too small", "gs_radix_sort_pairs");
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)div_up(n, kSortChunk);
  uint32_t *counts = (uint32_t *)workspace;
  uint32_t *totals = counts + (size_t)kRadix * nb;
  uint32_t *kin = keys, *vin = vals, *kout = keys_alt, *vout = vals_alt;
  // the bits spread evenly over the passes, the narrower digit first (13-bit
  // tile ids: 6 + 7, not 8 + 5): the first pass's scatter writes are the least
  // coalesced (its input is in emission order), so it gets the fewer, longer
  // digit runs per block (7 + 6 measured 0.9 us slower per scatter,
  // profiles/r05/sort_ab/)
  int shift = begin_bit;
  for (int p = 0; p < passes; ++p) {
    const int nbits = (end_bit - shift) / (passes - p);
    k_radix_hist<<<nb, kBlock, 0, s>>>(kin, n, shift, nbits, counts, nb, n_dev);
    k_radix_scan<<<1 << nbits, kBlock, 0, s>>>(counts, totals, nb, n_dev);
    if (p == 0 && vals_are_iota)
      k_radix_scatter<true><<<nb, kBlock, 0, s>>>(kin, nullptr, kout, vout, n, shift, nbits, counts, totals, nb,
                                                   n_dev);
    else
      k_radix_scatter<false><<<nb, kBlock, 0, s>>>(kin, vin, kout, vout, n, shift, nbits, counts, totals, nb,
                                                    n_dev);
    gs_status st = gs_internal_check_launch("gs_radix_sort_pairs");
    if (st) return st;
    shift += nbits;
    uint32_t *tk = kin, *tv = vin;
    kin = kout;
    vin = vout;
    kout = tk;
    vout = tv;
  }
  return GS_OK;
}

int32_t gs_internal_small_sort_max(void) { return kMsdCap; }

gs_status gs_internal_small_sort(const uint32_t *keys, const uint32_t *vals, uint32_t *keys_out, uint32_t *vals_out,
                                 int32_t n, int32_t bits, const uint32_t *n_dev, gs_stream_t stream) {
  if (n < 0 || n > kMsdCap || bits < 1 || bits > 32 || (n > 0 && (!keys || !keys_out || !vals_out)))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: bad args", "gs_internal_small_sort");
  if (n == 0) return GS_OK;
  k_msd_bucket_sort<true><<<1, kMsdThreads, 0, (hipStream_t)stream>>>(
      const_cast<uint32_t *>(keys), const_cast<uint32_t *>(vals), nullptr, bits, nullptr, (uint32_t)n, keys_out,
      vals_out, n_dev);
  return gs_internal_check_launch("gs_internal_small_sort");
}

extern "C" {

gs_status gs_depth_sort_msd(uint32_t *keys, uint32_t *vals, uint32_t *keys_alt, uint32_t *vals_alt, int32_t n,
                            int32_t key_bits, void *workspace, size_t workspace_bytes, uint32_t *overflow_word,
                            int32_t *result_in_alt, gs_stream_t stream) {
  if (!result_in_alt) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null result_in_alt", "gs_depth_sort_msd");
  if (key_bits < 9 || key_bits > 32 || n < 0)
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: key_bits must be 9..32", "gs_depth_sort_msd");
  *result_in_alt = 1;
  if (n == 0) return GS_OK;
  if (!keys || !vals || !keys_alt || !vals_alt || !workspace || !overflow_word ||
      workspace_bytes < gs_radix_sort_workspace_bytes(n))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer or workspace too small", "gs_depth_sort_msd");
  hipStream_t s = (hipStream_t)stream;
  const int nb = (int)div_up(n, kSortChunk);
  uint32_t *counts = (uint32_t *)workspace;
  uint32_t *totals = counts + (size_t)kRadix * nb;
  const int shift = key_bits - kRadixBits;
  k_radix_hist<<<nb, kBlock, 0, s>>>(keys, n, shift, kRadixBits, counts, nb);
  k_radix_scan<<<kRadix, kBlock, 0, s>>>(counts, totals, nb);
  k_radix_scatter<true><<<nb, kBlock, 0, s>>>(keys, nullptr, keys_alt, vals_alt, n, shift, kRadixBits, counts,
                                               totals, nb);
  k_msd_bucket_sort<false><<<kRadix - 1, kMsdThreads, 0, s>>>(keys_alt, vals_alt, totals, shift, overflow_word);
  return gs_internal_check_launch("gs_depth_sort_msd");
}

}  // extern "C"
