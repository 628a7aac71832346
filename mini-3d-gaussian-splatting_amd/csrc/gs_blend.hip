// gs_blend.hip -- the compositing kernels of the render path:
//   k_blend_fwd       renderer.py:273-367   per-pixel front-to-back compositing
//   k_blend_bwd       autograd of :313-367  replayed front-to-back, per-pair grad slots
// (src/core/renderer.py of the reference), the lane-statistics instantiation
// of the backward, and the size helpers of their buffers.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include <type_traits>

#include "gsplat_mi355x.h"
#include "gs_internal.h"
#include "gs_device.h"
#include "gs_blend_device.h"

namespace {

// torch.clamp semantics (NaN propagates)
__device__ __forceinline__ float clamp01(float v) { return v < 0.f ? 0.f : (v > 1.f ? 1.f : v); }
// wave-uniform "any lane" without the bool -> VGPR -> compare round trip
__device__ __forceinline__ bool wave_any(bool p) { return __builtin_amdgcn_ballot_w64(p) != 0; }

__device__ __forceinline__ uint32_t wave_max_u32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, d, 64));
  return v;
}

// Records staged in LDS are read as 8-byte pairs: ds_read_b64 costs 2 LDS
// cycles per wave-instruction (broadcast), ds_read_b96 8 and ds_read_b128 4
// (MI355X_MICROARCH.md, LDS table): (mx,my) (q00,qo) (q11,o) | (r,g) (b,z).
__device__ __forceinline__ float2 lds_pair(const float2 *p) {
  // volatile keeps each pair its own ds_read_b64 (no merging into b128 / read2)
  typedef __attribute__((address_space(3))) const volatile unsigned long long lds_u64;
  const unsigned long long v = *(lds_u64 *)(p);
  return make_float2(__uint_as_float((uint32_t)v), __uint_as_float((uint32_t)(v >> 32)));
}

// Wave-level culling of list entries: false only if every pixel centre of
// the 8x8 box [x0, x0 + 7] x [y0, y0 + 7] provably has s > 23.1, i.e.
// exp(-s/2) < 1e-5 (the :336 skip): the cell's wave may pass the entry over
// without evaluating it (each lane's own exact test still decides the rest).
// The s <= L ellipse, L = 23.1 * 1.01, lies in the box |x - mx| <= sqrt(L Sxx),
// |y - my| <= sqrt(L Syy), Sigma = Q^-1 for the form Q = [[q00, qo/2],
// [qo/2, q11]] the blend evaluates.  The 1% margin covers the fp32 rounding of
// s: |s_fp32 - s| <= ~4u (q00 dx^2 + |qo dx dy| + q11 dy^2) <= 4u (tr + |qo|)
// tr / det * s, so conics with (tr + |qo|) tr > 1e4 det -- and
// non-positive-definite or NaN ones -- are never culled.
__device__ __forceinline__ bool cell_hit(float mx, float my, float q00, float qo, float q11, float x0, float y0) {
  const float q01 = 0.5f * qo;
  const float det = q00 * q11 - q01 * q01, tr = q00 + q11;
  if (!(tr > 0.f && det > 0.f && (tr + fabsf(qo)) * tr <= 1e4f * det)) return true;
  const float L = 23.1f * 1.01f;
  // v_rcp / v_sqrt (~1 ulp): far inside the 1% margin
  const float id = __builtin_amdgcn_rcpf(det);
  const float hx = __builtin_amdgcn_sqrtf(L * q11 * id), hy = __builtin_amdgcn_sqrtf(L * q00 * id);
  const bool box = mx + hx >= x0 && mx - hx <= x0 + 7.f && my + hy >= y0 && my - hy <= y0 + 7.f;
  if (!box) return false;
  // The ellipse's bounding box meets the cell: the minimum of s over the
  // cell's box decides (a tilted, elongated ellipse's bounding box is much
  // larger than it).  The mean inside the box: s = 0.  Otherwise the minimum
  // lies on an edge: per edge the 1-D minimiser of the quadratic, clamped to
  // the edge.  A point of the box is evaluated, so the fp32 value is s at a
  // feasible point up to rounding -- the same ~4u (tr + |qo|) tr / det
  // relative error as above, inside the 1% margin.
  const float ax0 = x0 - mx, ax1 = x0 + 7.f - mx, ay0 = y0 - my, ay1 = y0 + 7.f - my;
  if (ax0 <= 0.f && ax1 >= 0.f && ay0 <= 0.f && ay1 >= 0.f) return true;
  const float kx = -0.5f * qo * __builtin_amdgcn_rcpf(q11), ky = -0.5f * qo * __builtin_amdgcn_rcpf(q00);
  auto sv = [&](float dx, float dy) { return (dx * dx) * q00 + (qo * dx) * dy + (dy * dy) * q11; };
  const float e0 = sv(ax0, __builtin_amdgcn_fmed3f(kx * ax0, ay0, ay1));
  const float e1 = sv(ax1, __builtin_amdgcn_fmed3f(kx * ax1, ay0, ay1));
  const float e2 = sv(__builtin_amdgcn_fmed3f(ky * ay0, ax0, ax1), ay0);
  const float e3 = sv(__builtin_amdgcn_fmed3f(ky * ay1, ax0, ax1), ay1);
  return fminf(fminf(e0, e1), fminf(e2, e3)) <= L;
}

// ======================================================== blend fwd =======
// Forward blend, one 64-lane workgroup per (tile, 8x8 cell), lane = pixel
// (compact footprints keep the per-pair branches coherent).  The cells of a
// tile run independently (no barrier): each stages its own batches of 64
// records in LDS (the next batch gathered into registers meanwhile), culls
// them against its own box (cell_hit, one ballot per batch) and walks the set
// bits.  Round 1 shared the staging between the four cells of a 16x16 tile
// in a 256-thread block and paid, at every barrier, for its busiest wave;
// here a cell's time is its own work, the records re-read per cell from the
// L2 the tile's cells share (8 us less at C3).  Control flow stays
// wave-uniform (ballots, scalar bit scans); per-lane decisions are
// predicates, and a skipped pair adds exact zeros: the :336 / :340 / :345
// skips are folded into the weight (a skipped pair gets ai = 0, hence
// c = (1 - A) * 0 = +0, and an accepted one c = (1 - A) * ai > 0 -- the
// reference's c exactly), v_cndmask selects instead of SGPR mask arithmetic.
// Each cell writes a liveness word per 64 entries for the backward
// (gs_blend_live_words).
// kCount: also count each pixel's contributing pairs (c > 0) into
// a.pair_counts -- a work counter for the measurement, off in the
// render path.  kT16: tile_size is the default 16 (its cell geometry folds to
// constants).
template <bool kCount, bool kT16>
__global__ __launch_bounds__(kWave) void k_blend_fwd(gs_blend_fwd_args a) {
  __shared__ float2 s_rec[kWave * 6];
  const CellGeom cg(kT16 ? GS_DEFAULT_TILE : a.cam.tile_size);
  const int ncell = cg.cells();
  int tile, quad;
  uint32_t start, end;
  cell_tile(blockIdx.x, ncell, a.ranges, a.tiles_x * a.tiles_y, (uint32_t)a.num_pairs, tile, quad, start, end);
  if (tile >= a.tiles_x * a.tiles_y) return;
  const int lane = threadIdx.x;
  const int cx0 = (quad % cg.QX) * 8, cy0 = (quad / cg.QX) * 8;  // the cell in its tile
  const int x0 = (tile % a.tiles_x) * cg.L + cx0, y0 = (tile / a.tiles_x) * cg.L + cy0;
  const int px = x0 + (lane & 7), py = y0 + (lane >> 3);
  const int W = a.cam.image_width, H = a.cam.image_height;
  const bool inside = cx0 + (lane & 7) < cg.L && cy0 + (lane >> 3) < cg.L && px < W && py < H;
  const float bg0 = a.cam.bg[0], bg1 = a.cam.bg[1], bg2 = a.cam.bg[2];
  float ar = bg0, ag = bg1, ab = bg2;  // out_rgb = bg (renderer.py:273)
  // a lane is done once A >= kAlphaStop (the :352 break); lanes outside the
  // tile or image start done
  float A = inside ? 0.f : 1.f, D = 0.f;
  uint32_t neval = 0, ncontrib = 0;
  // neval (1 + the last entry this lane evaluated while running, :352) is
  // kept lazily: `last` is that count for the running lanes of the last
  // evaluated entry (scalar), copied into a lane's neval only when it stops
  // (its bit leaves the running mask) -- two VALU less per evaluated entry
  uint32_t last = 0;
  unsigned long long runm = __builtin_amdgcn_ballot_w64(A < kAlphaStop);
  const float fx = (float)px, fy = (float)py;
  const float4 *recs = reinterpret_cast<const float4 *>(a.records);
  // liveness word of (this batch, this cell): see gs_blend_live_words
  // (no bitmap: the caller's budget; the backward then replays every entry)
  uint64_t *live = a.live_bits ? a.live_bits + (size_t)quad * a.live_words + start / 64u + (uint32_t)tile : nullptr;
  const uint64_t live_left = a.live_bits ? (uint64_t)a.live_words - (start / 64u + (uint32_t)tile) : 0u;
  float4 n0 = make_float4(0.f, 0.f, 0.f, 0.f), n1 = n0, n2 = n0;
  if (start + (uint32_t)lane < end) {
    const uint32_t gid = a.sorted_gauss[start + lane];
    n0 = recs[3 * (size_t)gid];
    n1 = recs[3 * (size_t)gid + 1];
    n2 = recs[3 * (size_t)gid + 2];
  }
  for (uint32_t b = start; b < end; b += kWave) {
    if (!wave_any(A < kAlphaStop)) break;  // every pixel of the cell done
    // stage the batch (this wave's own earlier reads precede these writes)
    float4 *d = reinterpret_cast<float4 *>(&s_rec[6 * lane]);
    d[0] = stage_conic0(n0);  // (the conic as -Q/2: the loop computes t = -s/2)
    d[1] = stage_conic1(n1);
    d[2] = n2;
    const bool hit = b + (uint32_t)lane < end && cell_hit(n0.x, n0.y, n0.z, n1.x, n0.w, (float)x0, (float)y0);
    const unsigned long long mw = __builtin_amdgcn_ballot_w64(hit);
    unsigned long long m = uniform_u64(mw);
    // the next batch's records in flight while this one composites
    // (fetching the ids a batch earlier, so that this is one round trip, was
    // measured: no change, profiles/r03/experiments.md)
    if (b + kWave + (uint32_t)lane < end) {
      const uint32_t gid = a.sorted_gauss[b + kWave + lane];
      n0 = recs[3 * (size_t)gid];
      n1 = recs[3 * (size_t)gid + 1];
      n2 = recs[3 * (size_t)gid + 2];
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the staged records, for every lane
    unsigned long long livem = 0;  // entries some lane of this cell evaluated
    // (packing the hits at compile-time offsets, round 6, so that the loop
    // needs no per-entry address move: no change, profiles/r06/exp5/)
    while (m) {
      const uint32_t bit = (uint32_t)__builtin_ctzll(m);
      m &= ~(1ull << bit);
      uint32_t ja;
      asm volatile("v_mov_b32 %0, %1" : "=v"(ja) : "s"(bit * 48u));
      const float2 *rj = reinterpret_cast<const float2 *>(reinterpret_cast<const char *>(s_rec) + ja);
      const float2 pm = lds_pair(rj), pq = lds_pair(rj + 1), po = lds_pair(rj + 2);
      const float dx = fx - pm.x, dy = fy - pm.y;
      const float t = conic_s(dx, dy, pq.x, po.x, pq.y);  // -s/2 (:333; conic staged as -Q/2)
      const bool run = A < kAlphaStop;
      const unsigned long long rm = __builtin_amdgcn_ballot_w64(run);  // (the compare's own SGPR result)
      const bool lv = run && !(t < kSkipT);  // the :336 skip, decided on s
      if (wave_any(lv)) {
        livem |= 1ull << bit;
        if (rm != runm) {  // lanes stopped since the last evaluated entry (rare)
          asm volatile("" ::: "memory");  // a real branch: not if-converted into every entry
          if ((runm >> lane) & 1ull) neval = last;
          runm = rm;
        }
        last = b - start + bit + 1;
        const float w = sat01(exp_blend(t));             // :334
        const float ai = lv ? sat01(po.y * w) : 0.f;      // :339 (skips folded into the weight)
        const float c = (1.f - A) * ai;                   // :343-344
        const float2 prg = lds_pair(rj + 3), pbz = lds_pair(rj + 4);
        ar = __builtin_fmaf(c, prg.x, ar);
        ag = __builtin_fmaf(c, prg.y, ag);
        ab = __builtin_fmaf(c, pbz.x, ab);
        A = A + c;
        D = __builtin_fmaf(c, pbz.y, D);
        if constexpr (kCount) ncontrib += c > 0.f ? 1u : 0u;
      }
    }
    const uint64_t wi = (b - start) / 64u;
    if (lane == 0 && wi < live_left) live[wi] = livem;
  }
  if ((runm >> lane) & 1ull) neval = last;
  if (inside && A < kAlphaStop) neval = end - start;
  // the cell's last evaluated entry (the backward replays up to it): lanes
  // outside the tile or image evaluated none
  const uint32_t cstop = wave_max_u32(inside ? neval : 0u);
  if (lane == 0) a.cell_neval[(size_t)tile * ncell + quad] = cstop;
  if (!inside) return;
  const size_t HW = (size_t)W * H, p = (size_t)py * W + px;
  const float tb = 1.f - A;
  const float pr = ar + tb * bg0, pg = ag + tb * bg1, pb = ab + tb * bg2;  // :359,364
  a.image[p] = clamp01(pr);
  a.image[HW + p] = clamp01(pg);
  a.image[2 * HW + p] = clamp01(pb);
  a.alpha[p] = clamp01(A);
  a.depth[p] = D / (A + 1e-6f);  // :362
  // The backward's per-pixel state is these outputs plus one byte: which
  // clamps blocked (value outside [0, 1], NaN included).  An unblocked
  // channel's image is the composite itself and A never leaves [0, 1] (each
  // step adds c <= 1 - A, rounded), so alpha is A.
  a.pix_flags[p] = (uint8_t)((pr >= 0.f && pr <= 1.f ? 0u : 1u) | (pg >= 0.f && pg <= 1.f ? 0u : 2u) |
                             (pb >= 0.f && pb <= 1.f ? 0u : 4u) | (A >= 0.f && A <= 1.f ? 0u : 8u));
  if (a.pix_neval) a.pix_neval[p] = neval;
  if constexpr (kCount) a.pair_counts[p] = ncontrib;
}

// ======================================================== blend bwd =======
// One 64-lane workgroup per (tile, 8x8 quadrant); lane = pixel, as in the
// forward's waves.  Nothing couples the four quadrants of a tile (no
// barrier): each walks only the list entries its own pixels evaluated in the
// forward (the liveness bitmap, exact), in list order, and writes one partial
// gradient per (entry, quadrant); gs_project_backward sums a slot's quadrant
// partials.
//  A (pixel-parallel), per live entry: replay the pixel's front-to-back chain
//    -- bit-identical to the forward's decisions -- and put two scalars per
//    pixel into a group buffer: dop = dL/d opacity and the contribution
//    weight c, whose sign bit flags exp(-s/2) > 1 (the weight clamp then
//    blocks dL/ds).
//  B (entry-parallel), per chunk of up to kBwdGroup live entries of a
//    64-entry word (records still staged): lanes 8j..8j+7 sum
//    entry j's 64 pixels -- lane 8j + x takes column x, rows 0..7 -- into the
//    10 gradient values and reduce them with 3 DPP steps.
// The records of a 64-entry word's live entries are gathered lane-parallel
// one word ahead (registers), staged in LDS and read back as broadcasts.
// live entries per phase-B group: 8, lanes 8j .. 8j + 7 on entry j (4 groups
// of 16 lanes: +85 us, tools/variants/README.md)
constexpr int kBwdGroup = 8;
constexpr int kBwdLanes = kWave / kBwdGroup;  // lanes per entry in phase B
// Group buffer rows (dop, c) are padded to 72 float2: phase B's lanes 8j + x
// read row j at pixel x + 8r, and 72 puts rows j = 0..3 of a 32-lane half on
// distinct banks (a stride of 64 would be a 4-way conflict).
constexpr int kBwdRow = kWave + 8;

// An entry whose clamps provably never bind: opacity in [1e-20, 1] and a
// conic passing cell_hit's conditioning test (positive definite, fp32 s >= 0
// at every pixel).  Then exp(-s/2) <= 1 and o w <= 1, and an accepted pair
// has c = (1 - A) o w >= 0.005 * 1e-20 * 1e-5 > 0.
__device__ __forceinline__ bool simple_entry(float4 r0, float4 r1) {
  const float q00 = r0.z, q11 = r0.w, qo = r1.x, o = r1.y;
  const float q01 = 0.5f * qo;
  const float det = q00 * q11 - q01 * q01, tr = q00 + q11;
  return o >= 1e-20f && o <= 1.f && tr > 0.f && det > 0.f && (tr + fabsf(qo)) * tr <= 1e4f * det;
}


// One launch replays the cells [cell_begin, cell_begin + cell_count) of every
// tile (the caller's batch: all of them unless a tile's cells would make the
// [T, cells] partial buffer too large; each batch's partials are summed by
// gs_gather_partials before the next batch overwrites them).  kT16: the
// default tile, one batch of its four cells.
// Phase-A lane statistics (gs_blend_backward_lane_stats; the kStats
// instantiation only -- the product kernel carries none of it): per replayed
// (entry, cell), the lanes still running into it and the lanes whose pair
// contributes (c > 0), as two 65-bin histograms, and per workgroup the
// replays, the replays entered with >= 32 running lanes, and the sums of
// running and contributing lanes.
struct BwdStats {
  unsigned long long *hist;  // [2][65]: running lanes, contributing lanes per replay
  uint32_t *per_group;       // [grid][4]
};

// Absolute screen-space gradients (gs_blend_backward_abs; the kAbs
// instantiations only -- the product kernel carries none of it): phase B also
// sums, per (entry, cell), |dL/dmu_x| and |dL/dmu_y| pixel by pixel -- the
// moments cannot give them, |.| of a linear form in (dx, dy) does not factor --
// and writes them as a float2 beside the 40-byte partial.
struct BwdAbs {
  float2 *grads;  // [T, G]: (sum_p |dL/dmu_x(p)|, sum_p |dL/dmu_y(p)|), flagged by slot_live
};

template <bool kT16, bool kStats = false, bool kAbs = false>
__global__ __launch_bounds__(kWave) void k_blend_bwd(gs_blend_bwd_args a, BwdStats stats = {nullptr, nullptr},
                                                     BwdAbs absg = {nullptr}) {
  __shared__ float2 s_dc[kBwdGroup][kBwdRow];  // per group entry and pixel: (dop, c)
  __shared__ uint32_t s_hist[kStats ? 2 * 65 : 1];
  uint32_t n_rep = 0, n_rep32 = 0, sum_run = 0, sum_con = 0;  // (kStats)
  if constexpr (kStats) {
    for (int i = threadIdx.x; i < 2 * 65; i += kWave) s_hist[i] = 0u;
    if (threadIdx.x < 4) stats.per_group[(size_t)blockIdx.x * 4 + threadIdx.x] = 0u;
  }
  __shared__ float4 s_pg[kWave];         // per pixel: dL/drgb (masked), dL/dD
  // the chunk's records (word 10 = slot), staged per chunk from registers:
  // 384 B instead of a word's 3 KB, for occupancy (LDS bounds it)
  __shared__ float2 s_wrec[kBwdGroup * 6];
  const CellGeom cg(kT16 ? GS_DEFAULT_TILE : a.cam.tile_size);
  const int ncell = kT16 ? cg.cells() : a.cell_count;  // partial groups of this batch
  const int cell0 = kT16 ? 0 : a.cell_begin;
  int tile, qb;
  uint32_t start, lend;
  cell_tile(blockIdx.x, ncell, a.ranges, a.tiles_x * a.tiles_y, (uint32_t)a.num_pairs, tile, qb, start, lend);
  if (tile >= a.tiles_x * a.tiles_y) return;
  const int quad = cell0 + qb;  // the cell in its tile; qb its partial group
  const int lane = threadIdx.x;
  const uint32_t tx = (uint32_t)(tile % a.tiles_x), ty = (uint32_t)(tile / a.tiles_x);
  const int cx0 = (quad % cg.QX) * 8, cy0 = (quad / cg.QX) * 8;  // the cell in its tile
  const int x0 = (int)tx * cg.L + cx0, y0 = (int)ty * cg.L + cy0;
  const int px = x0 + (lane & 7), py = y0 + (lane >> 3);
  const int W = a.cam.image_width, H = a.cam.image_height;
  const bool inside = cx0 + (lane & 7) < cg.L && cy0 + (lane >> 3) < cg.L && px < W && py < H;
  if (start >= lend) return;  // empty list: no gradient here (and no entry to read speculatively)
  const float4 *recs = reinterpret_cast<const float4 *>(a.records);
  // The prologue's loads in two round trips, without branches (a load under
  // a branch is waited for at its join): (1) the pixel's state and
  // cotangents, word 0's liveness word and its entries' Gaussian ids;
  // (2) speculatively every word-0 entry's record, not only the live ones.
  // Lanes outside the image / past the list read valid dummies (pixel 0,
  // entry 0), never used.
  // no bitmap (the caller's memory budget): every entry counts as live, and
  // the per-lane tests decide alone (slower, the same sums)
  const unsigned long long *lw =
      a.live_bits ? reinterpret_cast<const unsigned long long *>(a.live_bits) + (size_t)quad * a.live_words +
                        start / 64u + (uint32_t)tile
                  : nullptr;
  const unsigned long long w0 = lw ? lw[0] : ~0ull;
  const uint32_t gid0 = a.sorted_gauss[start + (uint32_t)lane < lend ? start + (uint32_t)lane : 0u];
  const size_t HW = (size_t)W * H;
  const size_t p = inside ? (size_t)py * W + px : 0;
  // the forward's outputs and clamp flags (k_blend_fwd): alpha is A, an
  // unblocked channel's image its composite
  const float im0 = a.image[p], im1 = a.image[HW + p], im2 = a.image[2 * HW + p];
  const float al = a.alpha[p], dep = a.depth[p];
  const uint32_t fl = a.pix_flags[p];
  const float gi0 = a.g_image[p], gi1 = a.g_image[HW + p], gi2 = a.g_image[2 * HW + p];
  const float gal = (a.g_alpha ? a.g_alpha : a.g_image)[p];
  const float gdp = (a.g_depth ? a.g_depth : a.g_image)[p];
  float4 r0 = recs[3 * (size_t)gid0], r1 = recs[3 * (size_t)gid0 + 1], r2 = recs[3 * (size_t)gid0 + 2];
  const float bg0 = a.cam.bg[0], bg1 = a.cam.bg[1], bg2 = a.cam.bg[2];
  // pixel cotangents through clamp / bg composite / depth normalisation
  // (selects, no branch: the compiler would sink the loads into it)
  const float At = inside ? al : 0.f;
  const float tb = 1.f - At;
  const float gR0 = (inside && !(fl & 1u)) ? gi0 : 0.f;
  const float gR1 = (inside && !(fl & 2u)) ? gi1 : 0.f;
  const float gR2 = (inside && !(fl & 4u)) ? gi2 : 0.f;
  // the accumulated colour without the background, where its gradient passes
  // (where it is blocked, gR = 0 and the value is not used)
  const float tr = inside ? im0 - tb * bg0 : 0.f, tg = inside ? im1 - tb * bg1 : 0.f;
  const float tbl = inside ? im2 - tb * bg2 : 0.f;
  const float Dt = inside ? dep * (At + 1e-6f) : 0.f;
  float gA = -gR0 * bg0 - gR1 * bg1 - gR2 * bg2;
  if (inside && a.g_alpha && !(fl & 8u)) gA += gal;
  const bool has_d = inside && a.g_depth;
  const float den = At + 1e-6f;
  const float gD = has_d ? gdp / den : 0.f;
  const float gAd = -gdp * Dt / (den * den);
  if (has_d) gA += gAd;
  // the cell's last evaluated entry: nothing past it carries gradient here
  const uint32_t wstop = __builtin_amdgcn_readfirstlane(a.cell_neval[(size_t)tile * cg.cells() + quad]);
  if (wstop == 0) return;
  s_pg[lane] = make_float4(gR0, gR1, gR2, gD);
  const float fx = (float)px, fy = (float)py;
  const float onemA = 1.f - At;
  // Suffix sums without per-channel state: with X_i = gR . col_i + gD z_i,
  //   sum_k gR_k (accT_k - acc_k) + gD (Dt - D) = K - P,
  //   K = gR . accT + gD Dt (per pixel),  P = gR . acc + gD D (running; acc starts at bg)
  // and dL/dalpha_i = T_i (X_i + (P - K + gA (1 - At)) / T_{i+1}) = T_i (X_i + (P + G0) / T_{i+1}).
  const float K = (gR0 * tr + gR1 * tg) + (gR2 * tbl + gD * Dt);
  const float G0 = __builtin_fmaf(gA, onemA, -K);
  // PG = P + G0 carried as one running sum (a gradient factor, no decision)
  float PG = ((gR0 * bg0 + gR1 * bg1) + gR2 * bg2) + G0;
  float A = 0.f, T1 = 1.f;  // T1 = 1 - A, carried: the next entry's transmittance is this one's rcp argument
  // running (A < 0.995 so far; lanes outside the image never run): replays
  // the forward's per-lane termination, so an entry past the pixel's n_eval
  // is never taken
  bool run = inside;
  const uint32_t nwords = (wstop + 63u) >> 6;
  // liveness word wd of this quadrant, cut at wstop (bits past it were never written)
  auto live_word = [&](uint32_t wd) -> unsigned long long {
    const unsigned long long w = wd == 0 ? w0 : (lw ? lw[wd] : ~0ull);
    const unsigned long long m = uniform_u64(w);
    const uint32_t rem = wstop - 64u * wd;
    return rem < 64u ? m & ((1ull << rem) - 1ull) : m;
  };
  // lane l gathers the record of entry 64 wd + l when that entry is live here
  auto fetch = [&](uint32_t wd, unsigned long long m) {
    if ((m >> lane) & 1ull) {
      const uint32_t gid = a.sorted_gauss[start + 64u * wd + (uint32_t)lane];
      r0 = recs[3 * (size_t)gid];
      r1 = recs[3 * (size_t)gid + 1];
      r2 = recs[3 * (size_t)gid + 2];
    }
  };
  // Phase B over a chunk: its k live entries, staged at s_wrec positions
  // 0 .. k - 1 (group order).
  auto phase_b = [&](auto masked_tag, int k) {
    constexpr bool kMasked = decltype(masked_tag)::value;
    // (the group buffer rows were written by this wave: waited for below)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int j = lane / kBwdLanes, col = lane % kBwdLanes;
    if (j < k) {
      const uint32_t e = (uint32_t)j;
      const float4 ia = reinterpret_cast<const float4 *>(s_wrec)[3 * e];  // mx my h00 h11 (h = -q/2)
      const float2 ib = s_wrec[6 * e + 2];                                // ho o
      const float q00 = -2.f * ia.z, q11 = -2.f * ia.w, qo = -2.f * ib.x;  // (exact)
      const uint32_t slot = __float_as_uint(s_wrec[6 * e + 5].x);
      const float hop = -0.5f * ib.y;
      // this lane's pixels (x0 + col, y0 + r): dx = bx, dy = by + (r - rc).
      // The row moments are taken about row rc of the column.  rc = 0 (moments
      // with constant weights r, r^2) unless the chunk holds a Gaussian with
      // sigma_y < 2 px: then rc is the column row nearest each mean (clamped),
      // else such a Gaussian's dy^2 sum cancels -- by^2 S0 + 2 by Soy + Soyy
      // with |by| up to 7 for a result of ~(0.05)^2 S0: 1e4 x fp32 rounding,
      // 1.7e-4 of the tensor's scale measured on a sub-pixel Gaussian (2e-6
      // recentred).  Always recentring cost +28 us per C3 step, this test +7.
      const float bx = (float)(x0 + col) - ia.x;
      const float q01h = 0.5f * qo;
      const bool small_y = q00 < 4.f * (q00 * q11 - q01h * q01h);  // Sigma_yy = q00 / det < 4
      float S0 = 0.f, Soy = 0.f, Soyy = 0.f, g5 = 0.f, g6 = 0.f, g7 = 0.f, g8 = 0.f, g9 = 0.f;
      float rc = 0.f;
      float ax = 0.f, ay = 0.f;  // (kAbs) sums of |ds| |d s / d mu| over the column's pixels
      const float qxx = 2.f * q00 * bx, qxy = qo * bx, q11x2 = 2.f * q11;  // (kAbs)
      auto moments = [&](auto recenter_tag) {
        constexpr bool kRec = decltype(recenter_tag)::value;
        if constexpr (kRec)
          rc = __builtin_amdgcn_fmed3f(__builtin_rintf(ia.y - (float)y0), 0.f, (float)(kBwdGroup - 1));
#pragma unroll
        for (int r = 0; r < kBwdGroup; ++r) {
          const int p = col + 8 * r;  // phase A's lane of that pixel
          const float2 dc = s_dc[j][p];
          const float dop = dc.x, cs = dc.y;
          const float4 pg = s_pg[p];
          // dL/ds = hop dop: none where the weight clamp bound (sign bit of c)
          // or the pair was skipped (dop = 0 then); a simple entry's clamps
          // never bind.  The moments are summed over dop and scaled by the
          // entry's hop once, after the rows (2 VALU less per row; unmasked,
          // the opacity sum g5 is the moment S0 itself)
          const float ds = kMasked ? (cs > 0.f ? dop : 0.f) : dop;
          const float cw = fabsf(cs);
          S0 += ds;
          if constexpr (kRec) {
            const float w = (float)r - rc;  // exact: small integers
            Soy = __builtin_fmaf(ds, w, Soy);
            Soyy = __builtin_fmaf(ds, w * w, Soyy);
          } else if (r) {
            Soy = __builtin_fmaf(ds, (float)r, Soy);
            Soyy = __builtin_fmaf(ds, (float)(r * r), Soyy);
          }
          if constexpr (kMasked) g5 += dop;
          if constexpr (kAbs) {
            // the pixel's own gradient, not through the moments: ds/dmu =
            // -(2 q00 dx + qo dy, qo dx + 2 q11 dy) at the forward's dy; no
            // recentring, nothing cancels in a sum of absolute values
            // (the empty asm keeps the row's terms in the row: hoisted out of the
            // unrolled loop, eight rows of them cost 17 VGPRs and a wave per SIMD)
            float yr = (float)(y0 + r);
            asm volatile("" : "+v"(yr));
            const float dyr = yr - ia.y;
            const float ads = fabsf(ds);
            ax = __builtin_fmaf(ads, fabsf(__builtin_fmaf(qo, dyr, qxx)), ax);
            ay = __builtin_fmaf(ads, fabsf(__builtin_fmaf(q11x2, dyr, qxy)), ay);
          }
          g6 = __builtin_fmaf(pg.x, cw, g6);
          g7 = __builtin_fmaf(pg.y, cw, g7);
          g8 = __builtin_fmaf(pg.z, cw, g8);
          g9 = __builtin_fmaf(pg.w, cw, g9);
        }
      };
      if (wave_any(small_y)) moments(std::true_type{}); else moments(std::false_type{});
      if constexpr (!kMasked) g5 = S0;
      S0 *= hop;
      Soy *= hop;
      Soyy *= hop;
      const float by = (float)y0 + rc - ia.y;
      // sums of ds dx, ds dy, ds dx^2, ds dx dy, ds dy^2 over the lane's column
      float Sx = bx * S0, Sy = __builtin_fmaf(by, S0, Soy);
      float g2 = bx * Sx, g3 = bx * Sy;
      float g4 = __builtin_fmaf(by, __builtin_fmaf(by, S0, 2.f * Soy), Soyy);
      Sx = oct_sum(Sx); Sy = oct_sum(Sy); g2 = oct_sum(g2); g3 = oct_sum(g3); g4 = oct_sum(g4);
      g5 = oct_sum(g5); g6 = oct_sum(g6); g7 = oct_sum(g7); g8 = oct_sum(g8); g9 = oct_sum(g9);
      if constexpr (kAbs) {
        const float ah = fabsf(hop);  // dL/ds = hop dop: scaled once, as the moments are
        ax = oct_sum(ax * ah);
        ay = oct_sum(ay * ah);
      }
      if (col == 0) {
        // dmu = -(2 q00 Sx + qo Sy, qo Sx + 2 q11 Sy)
        const float g0 = -(2.f * q00 * Sx + qo * Sy), g1 = -(qo * Sx + 2.f * q11 * Sy);
        const size_t sq = (size_t)slot * (uint32_t)ncell + (uint32_t)qb;
        // (dense 40-B partials, 8-B aligned: f4_u8)
        float *out = a.pair_grads + sq * GS_PARTIAL_STRIDE;
        *reinterpret_cast<f4_u8 *>(out) = f4_u8{g0, g1, g2, g3};
        *reinterpret_cast<f4_u8 *>(out + 4) = f4_u8{g4, g5, g6, g7};
        *reinterpret_cast<f2_u8 *>(out + 8) = f2_u8{g8, g9};
        if constexpr (kAbs) absg.grads[sq] = make_float2(ax, ay);
        a.slot_live[sq] = 1;
      }
    }
  };
  unsigned long long mcur = live_word(0);  // (word 0's records are in flight already)
  for (uint32_t wd = 0; wd < nwords; ++wd) {
    // word 10 of a live record becomes the entry's gradient slot (the
    // Gaussian's first slot + this tile's index in its rectangle)
    const bool mine = (mcur >> lane) & 1ull;
    const uint32_t info = __float_as_uint(r2.w);
    const uint32_t slot = __float_as_uint(r2.z) + (ty - ((info >> 12) & 0xFFFu)) * ((info >> 24) + 1u) +
                          (tx - (info & 0xFFFu));
    // packed: the live entry of rank r (bit order) at position r, so a
    // chunk's records sit at compile-time offsets from one base address
    const uint32_t rank =
        __builtin_amdgcn_mbcnt_hi((uint32_t)(mcur >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mcur, 0u));
    // this word's records stay in registers (staged chunk by chunk below)
    // while the next word's are fetched into r0..r2 (staging a whole word's
    // records, 3 KB of LDS, cost occupancy: -13 us when chunked)
    // (the conic staged as -Q/2: phase A computes t = -s/2; phase B undoes it)
    const float4 c0 = stage_conic0(r0), c1 = stage_conic1(r1), c2 = make_float4(r2.x, r2.y, __uint_as_float(slot), 0.f);
    const unsigned long long simple_w = __builtin_amdgcn_ballot_w64(mine && simple_entry(r0, r1));
    const unsigned long long mnext = wd + 1u < nwords ? live_word(wd + 1u) : 0ull;
    fetch(wd + 1u, mnext);  // in flight while this word replays
    // a word whose live entries are all simple (the common case) runs a copy
    // of the loop without the per-entry test
    auto run_word = [&](auto all_simple_tag) {
    constexpr bool kAllSimple = decltype(all_simple_tag)::value;
    unsigned long long m = mcur;
    uint32_t kb = 0;  // packed position of the chunk's first entry
    while (m) {
     // a chunk: the word's next (up to) kBwdGroup live entries
     unsigned long long cm = 0;
     int k = 0;
     // stage the chunk (ranks kb .. kb + kBwdGroup - 1; the previous chunk's
     // reads came before these writes in this wave's in-order LDS queue)
     if (mine && rank - kb < (uint32_t)kBwdGroup) {
       float4 *d = reinterpret_cast<float4 *>(&s_wrec[6 * (rank - kb)]);
       d[0] = c0;
       d[1] = c1;
       d[2] = c2;
     }
     asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the staged records, for every lane
     const char *cb = reinterpret_cast<const char *>(s_wrec);
     // unrolled: the group row k is a compile-time LDS offset
#pragma unroll
     for (int kk = 0; kk < kBwdGroup; ++kk) {
      if (kk > 0 && !m) break;
      const uint32_t bit = (uint32_t)__builtin_ctzll(m);
      m &= m - 1ull;
      cm |= 1ull << bit;
      // two b128 broadcasts and a b64: (mx my h00 h11) (ho o r g) (b z), h = -q/2;
      // pq = (h00, h11), po = (ho, opacity)
      const float4 r0v = reinterpret_cast<const float4 *>(cb + 48 * kk)[0];
      const float4 r1v = reinterpret_cast<const float4 *>(cb + 48 * kk)[1];
      const float2 pbz = reinterpret_cast<const float2 *>(cb + 48 * kk)[4];
      const float2 pm = make_float2(r0v.x, r0v.y), pq = make_float2(r0v.z, r0v.w);
      const float2 po = make_float2(r1v.x, r1v.y), prg = make_float2(r1v.z, r1v.w);
      const float dx = fx - pm.x, dy = fy - pm.y;
      const float tq = conic_s(dx, dy, pq.x, po.x, pq.y);  // -s/2, as in the forward
      // the w < 1e-5 skip on s, as in the forward (NaN falls through); `run`
      // is the forward's "A < 0.995 before this entry", carried from the
      // previous entry's own test -- the same decisions as i < n_eval
      const bool live = run && !(tq < kSkipT);
      uint32_t n_run = 0;
      if constexpr (kStats) n_run = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(run));
      const float X = __builtin_fmaf(gR0, prg.x, __builtin_fmaf(gR1, prg.y, __builtin_fmaf(gR2, pbz.x, gD * pbz.y)));
      const bool simple = kAllSimple || ((simple_w >> bit) & 1ull);
      float dop, cw;
      if (simple) {
        // Fast path (simple_entry): e = exp(-s/2) lies in [0, 1] (s >= 0) and
        // u = o w in [0, 1], so both clamps are identities and pass their
        // gradients -- the general path below with its clamp tests removed,
        // the same values.  wv = 0 exactly where the pair is skipped.
        const float w = exp_blend(tq);
        const float wv = live ? w : 0.f;
        const float trans = T1;
        const float c = trans * (po.y * wv);
        A = A + c;
        PG = __builtin_fmaf(c, X, PG);
        T1 = 1.f - A;
        const float inv = __builtin_amdgcn_rcpf(T1);  // v_rcp_f32 (1 ulp): a gradient factor, no decision
        const float d_live = __builtin_fmaf(inv, PG, X);
        // the terminating contributor has nothing behind it: (1-A_total)/T_{i+1} = 1
        const bool stop = !(A < kAlphaStop);
        const float dal = trans * (stop ? X + gA : d_live);
        run = run && !stop;
        dop = dal * wv;
        cw = c;
      } else {
        const float e = exp_blend(tq);
        const float w = sat01(e);
        const float u = po.y * w;
        const float ai = sat01(u);
        const float trans = T1;
        // the forward's skips folded into the weight exactly as there: c is
        // +0 for a skipped pair and > 0 for an accepted one (take <=> c > 0)
        const float c = trans * (live ? ai : 0.f);
        A = A + c;
        PG = __builtin_fmaf(c, X, PG);
        const bool term = !(A < kAlphaStop);
        T1 = 1.f - A;
        // both arms computed, then a select: no divergent branch per entry
        const float inv = __builtin_amdgcn_rcpf(T1);
        const float d_live = __builtin_fmaf(inv, PG, X);
        const float dal = trans * (term ? X + gA : d_live);
        run = run && !term;
        // u = o*w >= 0, so "u in [0,1]" (the clamp passes the gradient) is ai == u;
        // e = exp(.) >= 0, so "e in [0,1]" is w == e (both false for NaN)
        const float g = (ai == u) ? dal * w : 0.f;
        dop = (c > 0.f) ? g : 0.f;
        cw = (w == e) ? c : -c;  // c == +0 when skipped
      }
      s_dc[kk][lane] = make_float2(dop, cw);
      k = kk + 1;
      if constexpr (kStats) {
        const uint32_t n_con = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(cw != 0.f));
        if (lane == 0) {
          atomicAdd(&s_hist[n_run], 1u);
          atomicAdd(&s_hist[65 + n_con], 1u);
        }
        n_rep += 1u;
        n_rep32 += n_run >= 32u ? 1u : 0u;
        sum_run += n_run;
        sum_con += n_con;
      }
     }
     if (kAllSimple || (simple_w & cm) == cm) phase_b(std::false_type{}, k); else phase_b(std::true_type{}, k);
     kb += (uint32_t)k;
    }
    };
    if ((simple_w & mcur) == mcur) run_word(std::true_type{}); else run_word(std::false_type{});
    mcur = mnext;
  }
  if constexpr (kStats) {
    __syncthreads();
    if (lane == 0) {
      uint32_t *pg = stats.per_group + (size_t)blockIdx.x * 4;
      pg[0] = n_rep;
      pg[1] = n_rep32;
      pg[2] = sum_run;
      pg[3] = sum_con;
    }
    for (int i = lane; i < 2 * 65; i += kWave)
      if (s_hist[i]) atomicAdd(&stats.hist[i], (unsigned long long)s_hist[i]);
  }
}

// gs_blend_backward's checks, cell batch and launch; abs_grads: NULL, or the
// [T, G, 2] buffer of gs_blend_backward_abs (the kAbs instantiations)
gs_status blend_backward(const gs_blend_bwd_args *a, float *abs_grads, const char *what, gs_stream_t stream) {
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (!cam_ok(a->cam)) return gs_internal_fail(GS_ERR_UNSUPPORTED, kCamMsg, what);
  if (!tiles_match(a->cam, a->tiles_x, a->tiles_y))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: tiles_x/tiles_y do not match the image", what);
  if (!a->ranges || !a->sorted_gauss || !a->records || !a->image || !a->alpha || !a->depth || !a->pix_flags ||
      !a->cell_neval || !a->g_image ||
      !a->pair_grads || !a->slot_live || (a->live_bits && a->live_words <= 0))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", what);
  if (a->num_pairs < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative num_pairs", what);
  gs_blend_bwd_args b = *a;
  long long blocks;
  if (const gs_status st = cell_batch(b.cam.tile_size, b.tiles_x, b.tiles_y, b.cell_begin, b.cell_count, what, &blocks))
    return st;
  hipStream_t s = (hipStream_t)stream;
  const bool t16 = b.cam.tile_size == GS_DEFAULT_TILE && b.cell_count == cells_per_tile(b.cam.tile_size);
  if (abs_grads) {
    const BwdAbs ab{reinterpret_cast<float2 *>(abs_grads)};
    if (t16)
      k_blend_bwd<true, false, true><<<(unsigned)blocks, kWave, 0, s>>>(b, BwdStats{nullptr, nullptr}, ab);
    else
      k_blend_bwd<false, false, true><<<(unsigned)blocks, kWave, 0, s>>>(b, BwdStats{nullptr, nullptr}, ab);
  } else if (t16) {
    k_blend_bwd<true><<<(unsigned)blocks, kWave, 0, s>>>(b);
  } else {
    k_blend_bwd<false><<<(unsigned)blocks, kWave, 0, s>>>(b);
  }
  return gs_internal_check_launch(what);
}

}  // namespace

// ============================================================ C ABI =======
extern "C" {

int32_t gs_tile_quads(int32_t tile_size) {
  return (tile_size < 1 || tile_size > GS_MAX_TILE) ? 0 : cells_per_tile(tile_size);
}

int32_t gs_partial_groups(int32_t tile_size) {
  // one partial per 8x8 cell (a wave combining a tile's cells wrote fewer and
  // replayed slower: tools/variants/README.md)
  return (tile_size < 1 || tile_size > GS_MAX_TILE) ? 0 : cells_per_tile(tile_size);
}

size_t gs_blend_live_words(int32_t num_pairs, int32_t num_tiles) {
  if (num_pairs < 0 || num_tiles < 0) return 0;
  return (size_t)num_pairs / 64u + (size_t)num_tiles + 2u;
}

gs_status gs_blend_forward(const gs_blend_fwd_args *a, gs_stream_t stream) {
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", "gs_blend_forward");
  if (!cam_ok(a->cam)) return gs_internal_fail(GS_ERR_UNSUPPORTED, kCamMsg, "gs_blend_forward");
  if (!tiles_match(a->cam, a->tiles_x, a->tiles_y))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: tiles_x/tiles_y do not match the image", "gs_blend_forward");
  if (!a->ranges || !a->records || !a->image || !a->alpha || !a->depth || !a->pix_flags || !a->cell_neval ||
      (a->live_bits && a->live_words <= 0) || (a->num_pairs > 0 && !a->sorted_gauss))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", "gs_blend_forward");
  if (a->num_pairs < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative num_pairs", "gs_blend_forward");
  hipStream_t s = (hipStream_t)stream;
  const bool t16 = a->cam.tile_size == GS_DEFAULT_TILE;
  long long cblocks;
  if (!cell_grid(a->tiles_x, a->tiles_y, cells_per_tile(a->cam.tile_size), &cblocks))
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: too many tiles", "gs_blend_forward");
  if (a->pair_counts)
    k_blend_fwd<true, false><<<(unsigned)cblocks, kWave, 0, s>>>(*a);
  else if (t16)
    k_blend_fwd<false, true><<<(unsigned)cblocks, kWave, 0, s>>>(*a);
  else
    k_blend_fwd<false, false><<<(unsigned)cblocks, kWave, 0, s>>>(*a);
  return gs_internal_check_launch("gs_blend_forward");
}

gs_status gs_blend_backward(const gs_blend_bwd_args *a, gs_stream_t stream) {
  return blend_backward(a, nullptr, "gs_blend_backward", stream);
}

gs_status gs_blend_backward_abs(const gs_blend_bwd_args *a, float *abs_grads, gs_stream_t stream) {
  if (!abs_grads || (reinterpret_cast<uintptr_t>(abs_grads) & 7u))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: abs_grads must be an 8-byte aligned [T, G, 2] buffer",
                            "gs_blend_backward_abs");
  return blend_backward(a, abs_grads, "gs_blend_backward_abs", stream);
}

int64_t gs_blend_backward_groups(int32_t tiles_x, int32_t tiles_y, int32_t cell_count) {
  if (tiles_x <= 0 || tiles_y <= 0 || cell_count <= 0) return 0;
  return (int64_t)div_up(tiles_x * tiles_y, 8) * 8LL * cell_count;
}

gs_status gs_blend_backward_lane_stats(const gs_blend_bwd_args *a, uint64_t *hist, uint32_t *per_group,
                                       gs_stream_t stream) {
  if (!a || !hist || !per_group) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", "gs_blend_backward_lane_stats");
  if (a->cam.tile_size != GS_DEFAULT_TILE || !(a->cell_begin == 0 && (a->cell_count == 0 || a->cell_count == 4)))
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: the default tile, one batch", "gs_blend_backward_lane_stats");
  if (!a->ranges || !a->sorted_gauss || !a->records || !a->image || !a->alpha || !a->depth || !a->pix_flags ||
      !a->cell_neval || !a->g_image ||
      !a->pair_grads || !a->slot_live || !tiles_match(a->cam, a->tiles_x, a->tiles_y))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: bad buffers", "gs_blend_backward_lane_stats");
  gs_blend_bwd_args b = *a;
  b.cell_begin = 0;
  b.cell_count = 4;
  const int64_t blocks = gs_blend_backward_groups(b.tiles_x, b.tiles_y, 4);
  if (blocks <= 0) return GS_OK;
  hipStream_t s = (hipStream_t)stream;
  k_blend_bwd<true, true><<<(unsigned)blocks, kWave, 0, s>>>(
      b, BwdStats{reinterpret_cast<unsigned long long *>(hist), per_group});
  return gs_internal_check_launch("gs_blend_backward_lane_stats");
}

}  // extern "C"
