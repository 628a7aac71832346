// gs_blend_device.h -- what the blend family shares: the colour blend
// (gs_blend.hip) and the passes that replay it (gs_features.hip).  The one
// copy of everything that forms a blend decision -- the s skip, the weight
// c = (1 - A) sat(o sat(exp(-s/2))), A = A + c, T1 = 1 - A, the A >= 0.995
// stop -- so that a replay takes k_blend_fwd's decisions bit for bit by
// construction (both files are built with the same flags, no contraction),
// and of the cell geometry and the host checks of a cell launch.  Anonymous
// namespace, as gs_device.h; included by those two files only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

#include "gsplat_mi355x.h"
#include "gs_internal.h"
#include "gs_device.h"

namespace {

#ifndef GS_DEBUG  // 1: report (printf) blend list ranges clamped to the T entries
#define GS_DEBUG 0
#endif
constexpr float kAlphaStop = 0.995f;             // renderer.py:352
// renderer.py:336 skips a pair when w = exp(-s/2) < 1e-5; decided here on
// s: s > 2 ln(1e5).  The same decision except where exp's rounding
// straddles 1e-5 -- the band in which any two fp32 exps (ours, torch's)
// already disagree -- and it saves the compare on w for every evaluated
// pair (C3: the same 9 knife-edge pixels).  Forward and backward share it.
constexpr float kSkipS = 23.0258509f;
// The blend kernels evaluate t = -s/2 directly: the conic coefficients are
// staged as -Q/2 (a power-of-two scaling, exact for every product and sum of
// the reference's s), so the skip is t < -ln(1e5), the same decision.
constexpr float kSkipT = -0.5f * kSkipS;

// clamp to [0,1] as the VALU clamp output modifier (folds into the producing
// instruction).  Equals torch.clamp for every non-NaN input; NaN -> 0 instead
// of NaN (only reachable from NaN/inf inputs).  Used on the blend's hot path.
__device__ __forceinline__ float sat01(float v) { return __builtin_amdgcn_fmed3f(v, 0.f, 1.f); }

// exp(t) for the blend's exponent t = -s/2 (it evaluates the exp only for
// s <= 23.1, t in [-11.6, 0]; beyond, for non-positive-definite conics, it
// stays finite until 2^ph overflows), given t itself: the blend kernels
// compute t from the conic staged as -Q/2 (stage_conic0/1).  ph = t log2(e)
// rounded, 2^ph by v_exp_f32 (no range reduction or ldexp: 2^ph stays a
// normal float here), times (1 + d) with the remainder d = t - ph ln2 in
// natural-log units (Cody-Waite: ln2 in two parts, each fma's product exact).
// ~1 ulp, like expf; forward and backward share it, so their decisions
// replay bit-identically.  5 VALU per pair.  Rounds 2-5 took the remainder
// in log2 units (ph + pl from x log2(e), then 2^ph (1 + pl ln2)) and the
// exponent from s (x = -s/2): 6 VALU, and the same values (round 6: every one
// of 2.6 M sampled t, emulated).  Dropping the remainder's low part instead
// saves a VALU too, but is <= 3 ulp at t = -11.6: 12 knife-edge pixels and
// the scaling gradient's error 5.4e-4 -> 1.2e-3 of scale (round 2).  Not taken.
__device__ __forceinline__ float exp_blend(float t) {
  const float ph = t * 0x1.715476p+0f;
  const float r = __builtin_amdgcn_exp2f(ph);
  float d = __builtin_fmaf(-ph, 0x1.62e430p-1f, t);
  d = __builtin_fmaf(-ph, -0x1.05c610p-29f, d);
  return __builtin_fmaf(r, d, r);
}

// A record's conic staged for the blend loops as -Q/2: t = conic_s(dx, dy,
// h00, ho, h11) is then -s/2 exactly.
__device__ __forceinline__ float4 stage_conic0(float4 r0) {  // (mx, my, q00, q11) -> (mx, my, h00, h11)
  return make_float4(r0.x, r0.y, -0.5f * r0.z, -0.5f * r0.w);
}
__device__ __forceinline__ float4 stage_conic1(float4 r1) {  // (qo, o, r, g) -> (ho, o, r, g)
  return make_float4(-0.5f * r1.x, r1.y, r1.z, r1.w);
}

// s = [dx dy] Q [dx dy]^T for the blend's conic form (q00, qo = Q01+Q10,
// q11) in the reference's unfused order (renderer.py:333).  A fused form
// (5 operations instead of 8) was measured: with ill-conditioned conics the
// cancellation amplifies its ~1-ulp difference into visible errors (needle
// test: 1e-2 image error), so the reference's rounding is kept.
__device__ __forceinline__ float conic_s(float dx, float dy, float q00, float qo, float q11) {
  return ((dx * dx) * q00 + (qo * dx) * dy) + (dy * dy) * q11;
}

// The pair weight as a replay forms it, from t = -s/2, the opacity o, the
// pixel's T1 = 1 - A and `run` (the forward's "A < 0.995 before this entry"):
// the w < 1e-5 skip decided on s (NaN falls through), the two clamps, and the
// forward's skips folded into the weight exactly as there -- c is +0 for a
// skipped pair and > 0 for an accepted one (take <=> c > 0).  k_blend_fwd
// and k_blend_bwd spell the same operations inside their tuned loops.  A
// forward-type replay uses c alone; the backward ones also need the clamps'
// inputs: u = o w >= 0, so "u in [0,1]" (the clamp passes the gradient) is
// ai == u; e = exp(.) >= 0, so "e in [0,1]" is w == e (both false for NaN).
struct PairWeight {
  float e, w, u, ai, c;
  bool live;
};
__device__ __forceinline__ PairWeight pair_weight(float t, float o, float T1, bool run) {
  PairWeight p;
  p.live = run && !(t < kSkipT);        // the :336 skip
  p.e = exp_blend(t);
  p.w = sat01(p.e);                     // :334
  p.u = o * p.w;
  p.ai = sat01(p.u);                    // :339
  p.c = T1 * (p.live ? p.ai : 0.f);     // :343-344 (T1 = 1 - A)
  return p;
}
// The entry taken: A = A + c, T1 = 1 - A; false once A >= 0.995 (the :352
// break): the pixel takes no entry after this one.
__device__ __forceinline__ bool blend_advance(float &A, float &T1, float c) {
  A = A + c;
  T1 = 1.f - A;
  return A < kAlphaStop;
}

// Cells: a tile of edge L (GaussianRenderer.tile_size) is covered from its
// origin by QX x QX cells of 8x8 pixels, QX = ceil(L/8) (edge cells clipped
// to the tile); a wave renders one cell, lane l its pixel (l&7, l>>3), and
// blends the tile's whole list (renderer.py:302-319).  L = 16: the tile's
// four 8x8 quadrants.
struct CellGeom {
  int L, QX;
  __device__ explicit CellGeom(int tile_size) : L(tile_size), QX((tile_size + 7) >> 3) {}
  __device__ int cells() const { return QX * QX; }
};

// Workgroup b -> (tile, cell) and the tile's list range: b, b+8, b+16, ...
// share an XCD (round-robin dispatch; placement is for speed only), so the Q
// cells of a tile read its records through one L2.  Grid: ceil(tiles / 8) *
// 8 Q.  Position (b / 8 / Q) * 8 + b % 8 is the tile.  tile >= num_tiles:
// padding, no range.  (A heaviest-first dispatch order saved 4-9 us per
// launch at C3 but cost ~14 us to sort: tools/variants/README.md.)  The
// range is clamped to the T list entries (scalar, free): a corrupt ranges
// table cannot make the kernels read past sorted_gauss; a -DGS_DEBUG=1 build
// also reports any range it had to clamp.
__device__ __forceinline__ void cell_tile(uint32_t b, int ncell, const uint32_t *ranges, int ntiles, uint32_t T,
                                          int &tile, int &quad, uint32_t &start, uint32_t &end) {
  const uint32_t grp = b >> 3;
  const uint32_t q = (uint32_t)ncell;
  quad = (int)(grp % q);
  tile = (int)((grp / q) * 8u + (b & 7u));
  start = end = 0u;
  if (tile < ntiles) {
    start = __builtin_amdgcn_readfirstlane(ranges[2 * tile]);
    end = __builtin_amdgcn_readfirstlane(ranges[2 * tile + 1]);
#if GS_DEBUG
    if ((end > T || start > end) && threadIdx.x == 0)
      printf("gsplat: tile %d range [%u, %u) outside the %u entries, clamped\n", tile, start, end, T);
#endif
    end = min(end, T);
    start = min(start, end);
  }
}

__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long w) {
  // (readfirstlane returns int: widen through uint32_t, never sign-extend)
  return ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(w >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)w);
}

// Word 10 of a live record becomes the entry's gradient slot: the Gaussian's
// first slot + the index of tile (tx, ty) in its rectangle (word 11: the
// rectangle's first tile column and row, 12 bits each, and its width - 1).
__device__ __forceinline__ uint32_t entry_slot(float4 r2, uint32_t tx, uint32_t ty) {
  const uint32_t info = __float_as_uint(r2.w);
  return __float_as_uint(r2.z) + (ty - ((info >> 12) & 0xFFFu)) * ((info >> 24) + 1u) + (tx - (info & 0xFFFu));
}

// ---------------------------------------------------------- host checks ----
int cells_per_tile(int tile_size) {
  const int qx = (tile_size + GS_QUAD - 1) / GS_QUAD;
  return qx * qx;
}

bool tiles_match(const gs_camera &c, int tiles_x, int tiles_y) {
  return tiles_x == (int)div_up(c.image_width, c.tile_size) && tiles_y == (int)div_up(c.image_height, c.tile_size);
}

// The grid of a cell launch, cell_tile's: ceil(tiles / 8) * 8 workgroups for
// each of ncell cells, times `layers` (grid y).  False: too many -- a
// launch's work-items, workgroups x 64, must stay below 2^32.
bool cell_grid(int tiles_x, int tiles_y, int ncell, long long *blocks, long long layers = 1) {
  *blocks = (long long)div_up((long long)tiles_x * tiles_y, 8) * 8LL * ncell;
  return *blocks * layers * kWave <= 0xffffffffLL;
}

// A launch's cell batch [cell_begin, cell_begin + cell_count), defaulted
// (0, 0: every cell, one batch) and checked, and its grid.
gs_status cell_batch(int tile_size, int tiles_x, int tiles_y, int cell_begin, int32_t &cell_count,
                     const char *me, long long *blocks) {
  const int cells = cells_per_tile(tile_size);
  if (cell_count == 0 && cell_begin == 0) cell_count = cells;
  if (cell_begin < 0 || cell_count < 1 || cell_begin + cell_count > cells)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: the cell batch [cell_begin, cell_begin + cell_count) must lie in "
                "[0, gs_tile_quads(tile_size))", me);
  if (!cell_grid(tiles_x, tiles_y, cell_count, blocks))
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: too many tiles", me);
  return GS_OK;
}

}  // namespace
