// gs_features.hip -- per-Gaussian feature channels through the blend:
//   k_feat_fwd     features_out[k, p] = sum_i c_i F[g_i, k]   (the weights of renderer.py:319-353)
//   k_feat_bwd     its backward, per-pair grad slots in k_blend_bwd's layout
//   k_gather_feat  a chunk's partials summed per Gaussian (k_gather_slots' order)
//   k_contrib      per (entry, cell) the sum, max and count of c over the cell's pixels, and each
//                  pixel's strongest contributor; k_contrib_gather adds them up per Gaussian
//   k_dist_fwd     per pixel the depth distortion sum_ij c_i c_j |m_i - m_j| and the median entry
//   k_dist_bwd     the distortion's backward, per-pair grad slots in k_blend_bwd's layout
// No blend kernel here decides anything of its own: all replay the colour
// forward (k_blend_fwd, gs_blend.hip) over the state it saved -- ranges,
// sorted_gauss, records, cell_neval, live_bits -- with the operations
// k_blend_bwd replays it with.  The helpers that form a decision (exp_blend,
// conic_s, the -Q/2 staging, the s skip, A = A + c, T1 = 1 - A) are restated
// here from gs_blend.hip operation for operation: each .hip file is its own
// translation unit, built with the same flags (no contraction), so the same
// source gives the same bits.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsplat_mi355x.h"
#include "gs_internal.h"
#include "gs_device.h"

namespace {

constexpr float kAlphaStop = 0.995f;             // renderer.py:352
constexpr float kSkipS = 23.0258509f;            // renderer.py:336 on s: s > 2 ln(1e5)
constexpr float kSkipT = -0.5f * kSkipS;         // ... on t = -s/2

__device__ __forceinline__ float sat01(float v) { return __builtin_amdgcn_fmed3f(v, 0.f, 1.f); }

// gs_blend.hip's exp_blend (Cody-Waite around v_exp_f32), unchanged
__device__ __forceinline__ float exp_blend(float t) {
  const float ph = t * 0x1.715476p+0f;
  const float r = __builtin_amdgcn_exp2f(ph);
  float d = __builtin_fmaf(-ph, 0x1.62e430p-1f, t);
  d = __builtin_fmaf(-ph, -0x1.05c610p-29f, d);
  return __builtin_fmaf(r, d, r);
}

// t = -s/2 for a conic staged as -Q/2, in the reference's unfused order (renderer.py:333)
__device__ __forceinline__ float conic_s(float dx, float dy, float q00, float qo, float q11) {
  return ((dx * dx) * q00 + (qo * dx) * dy) + (dy * dy) * q11;
}

struct CellGeom {
  int L, QX;
  __device__ explicit CellGeom(int tile_size) : L(tile_size), QX((tile_size + 7) >> 3) {}
  __device__ int cells() const { return QX * QX; }
};

// Workgroup b -> (tile, cell of the launch's ncell) and the tile's list range,
// clamped to the T entries (k_blend_fwd's placement: b, b + 8, ... share an XCD).
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
    end = min(end, T);
    start = min(start, end);
  }
}

__device__ __forceinline__ unsigned long long uniform_u64(unsigned long long w) {
  // (readfirstlane returns int: widen through uint32_t, never sign-extend)
  return ((unsigned long long)(uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)(w >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((uint32_t)w);
}

// A cell's replay: its tile, pixel and the words of its liveness bitmap, cut
// at the cell's last evaluated entry (bits past it were never written).
struct Replay {
  int tile, quad, px, py;
  uint32_t tx, ty, start, wstop, nwords;
  int x0, y0;
  bool inside;
  const unsigned long long *lw;

  __device__ unsigned long long live_word(uint32_t wd) const {
    const unsigned long long m = uniform_u64(lw ? lw[wd] : ~0ull);
    const uint32_t rem = wstop - 64u * wd;
    return rem < 64u ? m & ((1ull << rem) - 1ull) : m;
  }
};

// false: nothing to replay (padding workgroup is reported through r.tile)
__device__ __forceinline__ bool replay_setup(Replay &r, const gs_camera &cam, int tiles_x, int tiles_y, int ncell,
                                             int cell0, const uint32_t *ranges, uint32_t T,
                                             const uint32_t *cell_neval, const uint64_t *live_bits,
                                             int64_t live_words) {
  const CellGeom cg(cam.tile_size);
  int qb;
  uint32_t end;
  cell_tile(blockIdx.x, ncell, ranges, tiles_x * tiles_y, T, r.tile, qb, r.start, end);
  r.wstop = r.nwords = 0u;
  r.inside = false;
  r.lw = nullptr;
  if (r.tile >= tiles_x * tiles_y) return false;
  r.quad = cell0 + qb;
  const int lane = threadIdx.x;
  r.tx = (uint32_t)(r.tile % tiles_x);
  r.ty = (uint32_t)(r.tile / tiles_x);
  const int cx0 = (r.quad % cg.QX) * 8, cy0 = (r.quad / cg.QX) * 8;  // the cell in its tile
  r.x0 = (int)r.tx * cg.L + cx0;
  r.y0 = (int)r.ty * cg.L + cy0;
  r.px = r.x0 + (lane & 7);
  r.py = r.y0 + (lane >> 3);
  r.inside = cx0 + (lane & 7) < cg.L && cy0 + (lane >> 3) < cg.L && r.px < cam.image_width && r.py < cam.image_height;
  if (r.start >= end) return false;
  // the cell's last evaluated entry (never past the list, whatever the word holds)
  r.wstop = min((uint32_t)__builtin_amdgcn_readfirstlane(cell_neval[(size_t)r.tile * cg.cells() + r.quad]),
                end - r.start);
  r.nwords = (r.wstop + 63u) >> 6;
  if (live_bits)
    r.lw = reinterpret_cast<const unsigned long long *>(live_bits) + (size_t)r.quad * live_words + r.start / 64u +
           (uint32_t)r.tile;
  return r.wstop != 0u;
}

// ====================================================== feature fwd =======
// One 64-lane workgroup per (tile, 8x8 cell) and chunk (grid y), lane = pixel.
// Per 64-entry word of the cell's liveness bitmap: the live entries' records
// and payloads are gathered lane-parallel (the next word's meanwhile, in
// registers), staged in LDS and walked in bit order as broadcasts.  The
// weight is k_blend_fwd's: skips folded in (a skipped pair gets ai = 0, hence
// c = +0), c = (1 - A) ai, A = A + c.
__global__ __launch_bounds__(kWave) void k_feat_fwd(gs_feature_fwd_args a) {
  __shared__ float4 s_rec[kWave * 3];  // per entry: (mx my h00 h11) (ho o - -) (f0 f1 f2 f3), h = -q/2
  Replay r;
  const CellGeom cg(a.cam.tile_size);
  const bool any = replay_setup(r, a.cam, a.tiles_x, a.tiles_y, cg.cells(), 0, a.ranges, (uint32_t)a.num_pairs,
                                a.cell_neval, a.live_bits, a.live_words);
  if (r.tile >= a.tiles_x * a.tiles_y) return;
  const int lane = threadIdx.x;
  const uint32_t chunk = blockIdx.y;
  const uint32_t ngauss = (uint32_t)a.num_gaussians;
  const float4 *recs = reinterpret_cast<const float4 *>(a.records);
  const float4 *feat = reinterpret_cast<const float4 *>(a.features) + (size_t)chunk * ngauss;
  float f0 = 0.f, f1 = 0.f, f2 = 0.f, f3 = 0.f;
  if (any) {
    const float fx = (float)r.px, fy = (float)r.py;
    float A = 0.f, T1 = 1.f;
    bool run = r.inside;  // A < 0.995 so far; lanes outside the tile or image never run
    float4 n0 = make_float4(0.f, 0.f, 0.f, 0.f), n1 = n0, nf = n0;
    auto fetch = [&](uint32_t wd, unsigned long long m) {
      if ((m >> lane) & 1ull) {
        const uint32_t gid = min(a.sorted_gauss[r.start + 64u * wd + (uint32_t)lane], ngauss - 1u);
        n0 = recs[3 * (size_t)gid];
        n1 = recs[3 * (size_t)gid + 1];
        nf = feat[gid];
      }
    };
    unsigned long long mcur = r.live_word(0);
    fetch(0, mcur);
    for (uint32_t wd = 0; wd < r.nwords; ++wd) {
      // (this wave's reads of the previous word precede these writes in its in-order LDS queue)
      if ((mcur >> lane) & 1ull) {
        s_rec[3 * lane] = make_float4(n0.x, n0.y, -0.5f * n0.z, -0.5f * n0.w);
        s_rec[3 * lane + 1] = make_float4(-0.5f * n1.x, n1.y, 0.f, 0.f);
        s_rec[3 * lane + 2] = nf;
      }
      const unsigned long long mnext = wd + 1u < r.nwords ? r.live_word(wd + 1u) : 0ull;
      fetch(wd + 1u, mnext);  // in flight while this word composites
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the staged records, for every lane
      unsigned long long m = mcur;
      while (m) {
        const uint32_t bit = (uint32_t)__builtin_ctzll(m);
        m &= m - 1ull;
        const float4 c0 = s_rec[3 * bit], c1 = s_rec[3 * bit + 1], fv = s_rec[3 * bit + 2];
        const float dx = fx - c0.x, dy = fy - c0.y;
        const float t = conic_s(dx, dy, c0.z, c1.x, c0.w);  // -s/2 (:333)
        const bool lv = run && !(t < kSkipT);                // the :336 skip, decided on s
        const float w = sat01(exp_blend(t));                 // :334
        const float ai = lv ? sat01(c1.y * w) : 0.f;         // :339
        const float c = T1 * ai;                             // :343-344 (T1 = 1 - A)
        f0 = __builtin_fmaf(c, fv.x, f0);
        f1 = __builtin_fmaf(c, fv.y, f1);
        f2 = __builtin_fmaf(c, fv.z, f2);
        f3 = __builtin_fmaf(c, fv.w, f3);
        A = A + c;
        T1 = 1.f - A;
        run = run && A < kAlphaStop;                         // the :352 break
      }
      asm volatile("" ::: "memory");
      mcur = mnext;
    }
  }
  if (!r.inside) return;
  const size_t HW = (size_t)a.cam.image_width * a.cam.image_height;
  const size_t p = (size_t)r.py * a.cam.image_width + r.px;
  const uint32_t ch = chunk * GS_FEATURE_CHUNK, C = (uint32_t)a.channels;
  a.out[(size_t)ch * HW + p] = f0;
  if (ch + 1u < C) a.out[(size_t)(ch + 1u) * HW + p] = f1;
  if (ch + 2u < C) a.out[(size_t)(ch + 2u) * HW + p] = f2;
  if (ch + 3u < C) a.out[(size_t)(ch + 3u) * HW + p] = f3;
}

// ====================================================== feature bwd =======
// k_blend_bwd's two phases over one chunk's payload, without its tuning (no
// simple-entry fast path, the row moments always recentred):
//  A (pixel-parallel), per live entry: replay the pixel's chain and put
//    (dop, c) into a group buffer; the sign bit of c flags exp(-s/2) > 1 (the
//    weight clamp then blocks dL/ds).
//  B (entry-parallel), per chunk of up to kBwdGroup live entries: lanes
//    8j..8j+7 sum entry j's 64 pixels -- lane 8j + x takes column x -- into
//    the 10 gradient values and reduce them with 3 DPP steps.
constexpr int kBwdGroup = 8;
constexpr int kBwdLanes = kWave / kBwdGroup;
constexpr int kBwdRow = kWave + 8;  // rows padded to 72 float2: no bank conflict between a half's rows

__global__ __launch_bounds__(kWave) void k_feat_bwd(gs_feature_bwd_args a) {
  __shared__ float2 s_dc[kBwdGroup][kBwdRow];  // per group entry and pixel: (dop, c)
  __shared__ float4 s_pg[kWave];               // per pixel: dL/dout of the chunk's four channels
  __shared__ float2 s_wrec[kBwdGroup * 6];     // the group's records: (mx my h00 h11) (ho o f0 f1) (f2 f3 slot -)
  Replay r;
  const int ncell = a.cell_count;
  if (!replay_setup(r, a.cam, a.tiles_x, a.tiles_y, ncell, a.cell_begin, a.ranges, (uint32_t)a.num_pairs,
                    a.cell_neval, a.live_bits, a.live_words))
    return;
  const int qb = r.quad - a.cell_begin;  // the cell's partial group
  const int lane = threadIdx.x;
  const uint32_t ngauss = (uint32_t)a.num_gaussians;
  const float4 *recs = reinterpret_cast<const float4 *>(a.records);
  const float4 *feat = reinterpret_cast<const float4 *>(a.features) + (size_t)a.chunk * ngauss;
  // the pixel's cotangents and outputs of this chunk (channels past C: zero;
  // lanes outside read pixel 0, unused)
  const size_t HW = (size_t)a.cam.image_width * a.cam.image_height;
  const size_t p = r.inside ? (size_t)r.py * a.cam.image_width + r.px : 0;
  const uint32_t ch = (uint32_t)a.chunk * GS_FEATURE_CHUNK, C = (uint32_t)a.channels;
  float gF[GS_FEATURE_CHUNK], oF[GS_FEATURE_CHUNK];
#pragma unroll
  for (uint32_t k = 0; k < GS_FEATURE_CHUNK; ++k) {
    const bool has = r.inside && ch + k < C;
    const size_t at = (size_t)min(ch + k, C - 1u) * HW + p;
    const float g = a.g_out[at], o = a.out[at];
    gF[k] = has ? g : 0.f;
    oF[k] = has ? o : 0.f;
  }
  s_pg[lane] = make_float4(gF[0], gF[1], gF[2], gF[3]);
  const float fx = (float)r.px, fy = (float)r.py;
  // dL/dalpha_i = T_i (X_i + (P_i - K) / T_{i+1}): PG = P - K carried as one
  // running sum (a gradient factor, no decision), P starts at 0 (no background)
  const float K = (gF[0] * oF[0] + gF[1] * oF[1]) + (gF[2] * oF[2] + gF[3] * oF[3]);
  float PG = -K;
  float A = 0.f, T1 = 1.f;
  bool run = r.inside;
  float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, rf = r0;
  auto fetch = [&](uint32_t wd, unsigned long long m) {
    if ((m >> lane) & 1ull) {
      const uint32_t gid = min(a.sorted_gauss[r.start + 64u * wd + (uint32_t)lane], ngauss - 1u);
      r0 = recs[3 * (size_t)gid];
      r1 = recs[3 * (size_t)gid + 1];
      r2 = recs[3 * (size_t)gid + 2];
      rf = feat[gid];
    }
  };
  // Phase B over a group: its k live entries, staged at s_wrec positions 0 .. k - 1.
  auto phase_b = [&](int k) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the group buffer rows this wave wrote
    const int j = lane / kBwdLanes, col = lane % kBwdLanes;
    if (j < k) {
      const uint32_t e = (uint32_t)j;
      const float4 ia = reinterpret_cast<const float4 *>(s_wrec)[3 * e];  // mx my h00 h11 (h = -q/2)
      const float2 ib = s_wrec[6 * e + 2];                                // ho o
      const float q00 = -2.f * ia.z, q11 = -2.f * ia.w, qo = -2.f * ib.x;  // (exact)
      const uint32_t slot = __float_as_uint(s_wrec[6 * e + 5].x);
      const float hop = -0.5f * ib.y;
      // this lane's pixels (x0 + col, y0 + row): dx = bx, dy = by + (row - rc).
      // The row moments are taken about the column row nearest the mean
      // (clamped), always: about row 0 the dy^2 sum of a Gaussian with
      // sigma_y << 1 px cancels (by^2 S0 + 2 by Soy + Soyy with |by| up to 7
      // for a result of ~sigma_y^2 S0), as k_blend_bwd's comment measures.
      const float bx = (float)(r.x0 + col) - ia.x;
      const float rc = __builtin_amdgcn_fmed3f(__builtin_rintf(ia.y - (float)r.y0), 0.f, (float)(kBwdGroup - 1));
      float S0 = 0.f, Soy = 0.f, Soyy = 0.f, g5 = 0.f, g6 = 0.f, g7 = 0.f, g8 = 0.f, g9 = 0.f;
#pragma unroll
      for (int row = 0; row < kBwdGroup; ++row) {
        const int pp = col + 8 * row;  // phase A's lane of that pixel
        const float2 dc = s_dc[j][pp];
        const float dop = dc.x, cs = dc.y;
        const float4 pg = s_pg[pp];
        // dL/ds = hop dop: none where the weight clamp bound (sign bit of c)
        // or the pair was skipped (dop = 0 then)
        const float ds = cs > 0.f ? dop : 0.f;
        const float cw = fabsf(cs);
        const float wr = (float)row - rc;  // exact: small integers
        S0 += ds;
        Soy = __builtin_fmaf(ds, wr, Soy);
        Soyy = __builtin_fmaf(ds, wr * wr, Soyy);
        g5 += dop;
        g6 = __builtin_fmaf(pg.x, cw, g6);
        g7 = __builtin_fmaf(pg.y, cw, g7);
        g8 = __builtin_fmaf(pg.z, cw, g8);
        g9 = __builtin_fmaf(pg.w, cw, g9);
      }
      S0 *= hop;
      Soy *= hop;
      Soyy *= hop;
      const float by = (float)r.y0 + rc - ia.y;
      // sums of ds dx, ds dy, ds dx^2, ds dx dy, ds dy^2 over the lane's column
      float Sx = bx * S0, Sy = __builtin_fmaf(by, S0, Soy);
      float g2 = bx * Sx, g3 = bx * Sy;
      float g4 = __builtin_fmaf(by, __builtin_fmaf(by, S0, 2.f * Soy), Soyy);
      Sx = oct_sum(Sx); Sy = oct_sum(Sy); g2 = oct_sum(g2); g3 = oct_sum(g3); g4 = oct_sum(g4);
      g5 = oct_sum(g5); g6 = oct_sum(g6); g7 = oct_sum(g7); g8 = oct_sum(g8); g9 = oct_sum(g9);
      if (col == 0) {
        // dmu = -(2 q00 Sx + qo Sy, qo Sx + 2 q11 Sy)
        const float g0 = -(2.f * q00 * Sx + qo * Sy), g1 = -(qo * Sx + 2.f * q11 * Sy);
        const size_t sq = (size_t)slot * (uint32_t)ncell + (uint32_t)qb;
        if (slot < (uint32_t)a.num_pairs) {  // (a slot of this frame's T; a corrupt record writes nothing)
          float *out = a.pair_grads + sq * GS_PARTIAL_STRIDE;  // (dense 40-B partials, 8-B aligned: f4_u8)
          *reinterpret_cast<f4_u8 *>(out) = f4_u8{g0, g1, g2, g3};
          *reinterpret_cast<f4_u8 *>(out + 4) = f4_u8{g4, g5, g6, g7};
          *reinterpret_cast<f2_u8 *>(out + 8) = f2_u8{g8, g9};
          a.slot_live[sq] = 1;
        }
      }
    }
  };
  unsigned long long mcur = r.live_word(0);
  fetch(0, mcur);
  for (uint32_t wd = 0; wd < r.nwords; ++wd) {
    // word 10 of a live record becomes the entry's gradient slot (the
    // Gaussian's first slot + this tile's index in its rectangle)
    const bool mine = (mcur >> lane) & 1ull;
    const uint32_t info = __float_as_uint(r2.w);
    const uint32_t slot = __float_as_uint(r2.z) + (r.ty - ((info >> 12) & 0xFFFu)) * ((info >> 24) + 1u) +
                          (r.tx - (info & 0xFFFu));
    // packed: the live entry of rank k (bit order) at position k of its group
    const uint32_t rank =
        __builtin_amdgcn_mbcnt_hi((uint32_t)(mcur >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mcur, 0u));
    // (the conic staged as -Q/2: phase A computes t = -s/2; phase B undoes it)
    const float4 c0 = make_float4(r0.x, r0.y, -0.5f * r0.z, -0.5f * r0.w);
    const float4 c1 = make_float4(-0.5f * r1.x, r1.y, rf.x, rf.y);
    const float4 c2 = make_float4(rf.z, rf.w, __uint_as_float(slot), 0.f);
    const unsigned long long mnext = wd + 1u < r.nwords ? r.live_word(wd + 1u) : 0ull;
    fetch(wd + 1u, mnext);  // in flight while this word replays
    unsigned long long m = mcur;
    uint32_t kb = 0;  // packed position of the group's first entry
    while (m) {
      int k = 0;
      // stage the group (ranks kb .. kb + kBwdGroup - 1; the previous group's
      // reads came before these writes in this wave's in-order LDS queue)
      if (mine && rank - kb < (uint32_t)kBwdGroup) {
        float4 *d = reinterpret_cast<float4 *>(&s_wrec[6 * (rank - kb)]);
        d[0] = c0;
        d[1] = c1;
        d[2] = c2;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the staged records, for every lane
      const char *cb = reinterpret_cast<const char *>(s_wrec);
#pragma unroll
      for (int kk = 0; kk < kBwdGroup; ++kk) {
        if (kk > 0 && !m) break;
        m &= m - 1ull;
        const float4 r0v = reinterpret_cast<const float4 *>(cb + 48 * kk)[0];
        const float4 r1v = reinterpret_cast<const float4 *>(cb + 48 * kk)[1];
        const float2 f23 = reinterpret_cast<const float2 *>(cb + 48 * kk)[4];
        const float dx = fx - r0v.x, dy = fy - r0v.y;
        const float tq = conic_s(dx, dy, r0v.z, r1v.x, r0v.w);  // -s/2, as in the forward
        // `run` is the forward's "A < 0.995 before this entry", carried from
        // the previous entry's own test
        const bool live = run && !(tq < kSkipT);
        const float X = __builtin_fmaf(gF[0], r1v.z, __builtin_fmaf(gF[1], r1v.w, __builtin_fmaf(gF[2], f23.x, gF[3] * f23.y)));
        const float e = exp_blend(tq);
        const float w = sat01(e);
        const float u = r1v.y * w;
        const float ai = sat01(u);
        const float trans = T1;
        // the forward's skips folded into the weight exactly as there: c is
        // +0 for a skipped pair and > 0 for an accepted one
        const float c = trans * (live ? ai : 0.f);
        A = A + c;
        PG = __builtin_fmaf(c, X, PG);
        const bool term = !(A < kAlphaStop);
        T1 = 1.f - A;
        // both arms computed, then a select: no divergent branch per entry
        const float inv = __builtin_amdgcn_rcpf(T1);  // v_rcp_f32 (1 ulp): a gradient factor, no decision
        const float d_live = __builtin_fmaf(inv, PG, X);
        // the terminating contributor has nothing behind it
        const float dal = trans * (term ? X : d_live);
        run = run && !term;
        // u = o w >= 0, so "u in [0,1]" (the clamp passes the gradient) is ai == u;
        // e = exp(.) >= 0, so "e in [0,1]" is w == e (both false for NaN)
        const float g = (ai == u) ? dal * w : 0.f;
        const float dop = (c > 0.f) ? g : 0.f;
        const float cw = (w == e) ? c : -c;  // c == +0 when skipped
        s_dc[kk][lane] = make_float2(dop, cw);
        k = kk + 1;
      }
      phase_b(k);
      kb += (uint32_t)k;
    }
    mcur = mnext;
  }
}

// ========================================================== gather ========
// k_gather_slots' walk (gs_project.hip): QL x HL lanes per Gaussian, lane
// (h, q) adds the live partials of g's slots h, h + HL, ... for the partial
// groups q, q + QL, ..., then the lane sums are added in the same DPP order.
template <int LPG>
__device__ __forceinline__ float lanes_sum(float v) {
  if constexpr (LPG == 8) return oct_sum(v);
  if constexpr (LPG == 4 || LPG == 2) {
    v += dpp_row<0xB1>(v);  // quad_perm [1,0,3,2]
    if constexpr (LPG == 4) v += dpp_row<0x4E>(v);  // quad_perm [2,3,0,1]
    asm volatile("" : "+v"(v));
  }
  return v;
}

template <int QL, int HL>
__global__ __launch_bounds__(kBlock) void k_gather_feat(gs_feature_gather_args a) {
  constexpr int LPG = QL * HL;
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int g = (int)(t / LPG);
  const int h = (int)((t % LPG) / QL), q = (int)(t % QL);
  float acc[GS_PAIR_GRAD_FLOATS];
#pragma unroll
  for (int k = 0; k < GS_PAIR_GRAD_FLOATS; ++k) acc[k] = 0.f;
  const bool valid = g < a.n;
  const uint32_t gi = valid ? (uint32_t)g : 0u;
  const uint2 rect = reinterpret_cast<const uint2 *>(a.rects)[gi];
  const int tx0 = (int)(rect.x & 0xFFFFu), tx1 = (int)(rect.x >> 16);
  const int ty0 = (int)(rect.y & 0xFFFFu), ty1 = (int)(rect.y >> 16);
  const size_t off = a.pair_offset[gi];
  const uint32_t cnt = (valid && a.vis[gi]) ? rect_touches(tx0, tx1, ty0, ty1) : 0u;
  const uint32_t ng = (uint32_t)a.partial_groups;
  for (uint32_t qc = (uint32_t)q; qc < ng; qc += QL) {
    for (uint32_t e = (uint32_t)h; e < cnt; e += HL) {
      const size_t at = (off + e) * ng + qc;
      if (!a.slot_live[at]) continue;
      const float *src = a.pair_grads + at * GS_PARTIAL_STRIDE;
      const f4_u8 va = *reinterpret_cast<const f4_u8 *>(src), vb = *reinterpret_cast<const f4_u8 *>(src + 4);
      const f2_u8 vc = *reinterpret_cast<const f2_u8 *>(src + 8);
      acc[0] += va.x; acc[1] += va.y; acc[2] += va.z; acc[3] += va.w;
      acc[4] += vb.x; acc[5] += vb.y; acc[6] += vb.z; acc[7] += vb.w;
      acc[8] += vc.x; acc[9] += vc.y;
    }
  }
#pragma unroll
  for (int k = 0; k < GS_PAIR_GRAD_FLOATS; ++k) acc[k] = lanes_sum<LPG>(acc[k]);
  if ((t % LPG) != 0 || !valid) return;
  float *gs = a.grad_sums + (size_t)g * GS_PAIR_GRAD_FLOATS;
  if (a.accumulate) {
#pragma unroll
    for (int k = 0; k < 6; ++k) gs[k] += acc[k];
  } else {
#pragma unroll
    for (int k = 0; k < 6; ++k) gs[k] = acc[k];
#pragma unroll
    for (int k = 6; k < GS_PAIR_GRAD_FLOATS; ++k) gs[k] = 0.f;
  }
  float *df = a.d_features + (size_t)g * a.d_features_stride + a.channel_begin;
#pragma unroll
  for (int k = 0; k < GS_FEATURE_CHUNK; ++k)
    if (k < a.channel_count) df[k] = a.feature_accumulate ? df[k] + acc[6 + k] : acc[6 + k];
}

// ==================================================== contributions =======
// A third replay, with no payload: how much every entry contributes.
//  A (pixel-parallel), per live entry: the pixel's c into a group buffer,
//    and the pixel's largest c so far with its Gaussian (strict >: the first
//    entry in list order wins).
//  B (entry-parallel), per group of up to kBwdGroup live entries: lanes
//    8j..8j+7 reduce entry j's 64 pixels -- lane 8j + x takes column x, rows
//    0..7 in order -- to (sum, max, count) and finish with 3 DPP steps each.
constexpr int kCtbRow = kWave + 8;  // rows padded to 72 floats: the 8 entries' columns fall in 64 different banks

__device__ __forceinline__ float oct_max(float v) {
  v = fmaxf(v, dpp_row<0xB1>(v));
  v = fmaxf(v, dpp_row<0x4E>(v));
  v = fmaxf(v, dpp_row<0x141>(v));
  return v;
}

__global__ __launch_bounds__(kWave) void k_contrib(gs_contrib_args a) {
  __shared__ float s_c[kBwdGroup][kCtbRow];  // per group entry and pixel: c
  __shared__ float4 s_wrec[kBwdGroup * 2];   // the group's records: (mx my h00 h11) (ho o slot gid)
  Replay r;
  const int ncell = a.cell_count;
  const bool any = replay_setup(r, a.cam, a.tiles_x, a.tiles_y, ncell, a.cell_begin, a.ranges,
                                (uint32_t)a.num_pairs, a.cell_neval, a.live_bits, a.live_words);
  if (r.tile >= a.tiles_x * a.tiles_y) return;
  const int lane = threadIdx.x;
  float best = 0.f;
  int best_id = -1;
  if (any) {
    const int qb = r.quad - a.cell_begin;  // the cell's partial group
    const uint32_t ngauss = (uint32_t)a.num_gaussians;
    const float4 *recs = reinterpret_cast<const float4 *>(a.records);
    const float fx = (float)r.px, fy = (float)r.py;
    float A = 0.f, T1 = 1.f;
    bool run = r.inside;
    float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0;
    uint32_t gcur = 0u;
    auto fetch = [&](uint32_t wd, unsigned long long m) {
      if ((m >> lane) & 1ull) {
        gcur = min(a.sorted_gauss[r.start + 64u * wd + (uint32_t)lane], ngauss - 1u);
        r0 = recs[3 * (size_t)gcur];
        r1 = recs[3 * (size_t)gcur + 1];
        r2 = recs[3 * (size_t)gcur + 2];
      }
    };
    auto phase_b = [&](int k) {
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the group buffer rows this wave wrote
      const int j = lane / kBwdLanes, col = lane % kBwdLanes;
      if (j < k) {
        float sum = 0.f, mx = 0.f, cnt = 0.f;
#pragma unroll
        for (int row = 0; row < kBwdGroup; ++row) {
          const float c = s_c[j][col + 8 * row];
          sum += c;
          mx = fmaxf(mx, c);
          cnt += c > 0.f ? 1.f : 0.f;
        }
        sum = oct_sum(sum);
        mx = oct_max(mx);
        cnt = oct_sum(cnt);  // (small integers: exact)
        if (col == 0) {
          const uint32_t slot = __float_as_uint(s_wrec[2 * j + 1].z);
          if (slot < (uint32_t)a.num_pairs) {  // (a slot of this frame's T; a corrupt record writes nothing)
            const size_t sq = (size_t)slot * (uint32_t)ncell + (uint32_t)qb;
            reinterpret_cast<float4 *>(a.partials)[sq] = make_float4(sum, mx, cnt, 0.f);
            a.slot_live[sq] = 1;
          }
        }
      }
    };
    unsigned long long mcur = r.live_word(0);
    fetch(0, mcur);
    for (uint32_t wd = 0; wd < r.nwords; ++wd) {
      // the entry's gradient slot, as k_feat_bwd forms it
      const bool mine = (mcur >> lane) & 1ull;
      const uint32_t info = __float_as_uint(r2.w);
      const uint32_t slot = __float_as_uint(r2.z) + (r.ty - ((info >> 12) & 0xFFFu)) * ((info >> 24) + 1u) +
                            (r.tx - (info & 0xFFFu));
      const uint32_t rank =
          __builtin_amdgcn_mbcnt_hi((uint32_t)(mcur >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mcur, 0u));
      const float4 c0 = make_float4(r0.x, r0.y, -0.5f * r0.z, -0.5f * r0.w);
      const float4 c1 = make_float4(-0.5f * r1.x, r1.y, __uint_as_float(slot), __uint_as_float(gcur));
      const unsigned long long mnext = wd + 1u < r.nwords ? r.live_word(wd + 1u) : 0ull;
      fetch(wd + 1u, mnext);  // in flight while this word replays
      unsigned long long m = mcur;
      uint32_t kb = 0;  // packed position of the group's first entry
      while (m) {
        int k = 0;
        // (the previous group's reads came before these writes in this wave's in-order LDS queue)
        if (mine && rank - kb < (uint32_t)kBwdGroup) {
          s_wrec[2 * (rank - kb)] = c0;
          s_wrec[2 * (rank - kb) + 1] = c1;
        }
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the staged records, for every lane
#pragma unroll
        for (int kk = 0; kk < kBwdGroup; ++kk) {
          if (kk > 0 && !m) break;
          m &= m - 1ull;
          const float4 r0v = s_wrec[2 * kk], r1v = s_wrec[2 * kk + 1];
          const float dx = fx - r0v.x, dy = fy - r0v.y;
          const float t = conic_s(dx, dy, r0v.z, r1v.x, r0v.w);  // -s/2, as in the forward
          const bool lv = run && !(t < kSkipT);
          const float w = sat01(exp_blend(t));
          const float ai = lv ? sat01(r1v.y * w) : 0.f;
          const float c = T1 * ai;
          if (c > best) {
            best = c;
            best_id = (int)__float_as_uint(r1v.w);
          }
          A = A + c;
          T1 = 1.f - A;
          run = run && A < kAlphaStop;
          s_c[kk][lane] = c;
          k = kk + 1;
        }
        phase_b(k);
        kb += (uint32_t)k;
      }
      mcur = mnext;
    }
  }
  if (a.dominant_id && r.inside) {
    const size_t p = (size_t)r.py * a.cam.image_width + r.px;
    a.dominant_id[p] = best_id;
    a.dominant_weight[p] = best;
  }
}

__global__ __launch_bounds__(kBlock) void k_contrib_empty(int32_t *id, float *weight, long long pixels) {
  const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (p < pixels) {
    id[p] = -1;
    weight[p] = 0.f;
  }
}

template <int LPG>
__device__ __forceinline__ float lanes_max(float v) {
  if constexpr (LPG == 8) return oct_max(v);
  if constexpr (LPG == 4 || LPG == 2) {
    v = fmaxf(v, dpp_row<0xB1>(v));
    if constexpr (LPG == 4) v = fmaxf(v, dpp_row<0x4E>(v));
  }
  return v;
}

// k_gather_feat's walk and lane tree over the 16-byte contribution partials
template <int QL, int HL>
__global__ __launch_bounds__(kBlock) void k_contrib_gather(gs_contrib_gather_args a) {
  constexpr int LPG = QL * HL;
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int g = (int)(t / LPG);
  const int h = (int)((t % LPG) / QL), q = (int)(t % QL);
  const bool valid = g < a.n;
  const uint32_t gi = valid ? (uint32_t)g : 0u;
  const bool seen = valid && a.vis[gi];
  const uint2 rect = reinterpret_cast<const uint2 *>(a.rects)[gi];
  const int tx0 = (int)(rect.x & 0xFFFFu), tx1 = (int)(rect.x >> 16);
  const int ty0 = (int)(rect.y & 0xFFFFu), ty1 = (int)(rect.y >> 16);
  const size_t off = a.pair_offset[gi];
  const uint32_t cnt = seen ? rect_touches(tx0, tx1, ty0, ty1) : 0u;
  const uint32_t ng = (uint32_t)a.partial_groups;
  float s = 0.f, m = 0.f;
  int ki = 0;  // (counts as integers: a Gaussian's total may pass 2^24)
  for (uint32_t qc = (uint32_t)q; qc < ng; qc += QL) {
    for (uint32_t e = (uint32_t)h; e < cnt; e += HL) {
      const size_t at = (off + e) * ng + qc;
      if (!a.slot_live[at]) continue;
      const float4 v = reinterpret_cast<const float4 *>(a.partials)[at];
      s += v.x;
      m = fmaxf(m, v.y);
      ki += (int)v.z;
    }
  }
  s = lanes_sum<LPG>(s);
  m = lanes_max<LPG>(m);
  ki += __builtin_amdgcn_update_dpp(0, ki, 0xB1, 0xF, 0xF, true);
  if constexpr (LPG >= 4) ki += __builtin_amdgcn_update_dpp(0, ki, 0x4E, 0xF, 0xF, true);
  if constexpr (LPG == 8) ki += __builtin_amdgcn_update_dpp(0, ki, 0x141, 0xF, 0xF, true);
  if ((t % LPG) != 0 || !seen) return;
  a.weight_sum[g] = a.weight_sum[g] + s;
  a.weight_max[g] = fmaxf(a.weight_max[g], m);
  a.pixels[g] += (int64_t)ki;
  a.views[g] += a.first_batch ? 1 : 0;
}

// ================================================= depth distortion =======
// A fourth replay, with a pairwise payload: per pixel
//   distortion = sum_i sum_j c_i c_j |m_i - m_j| = 2 sum_i c_i (m_i A_{i-1} - S_{i-1}),
//   A_i = sum_{j<=i} c_j,  S_i = sum_{j<=i} c_j m_j
// (the lists are sorted by the bits of z and both depth maps are monotone, so
// the prefix form is the double sum), and the median entry: the first with
// c > 0 after whose addition the running A >= 0.5, else the last with c > 0.
// The sum does not change under a shift common to all m, and in fp32 it needs
// one: the kernels work on differences to the pixel's first contributor f,
//   m_i = (z_i - z_f) q_i r_f,   linear: q = r = 1;  inverse: q = kappa / z, r = 1 / z
// (kappa (z_i - z_f) / (z_i z_f) is 2DGS's NDC depth far (z - near) / ((far - near) z)
// minus its value at z_f), formed from the record depths directly: z_i - z_f
// is exact or one rounding of a value no larger than the pixel's own depth
// spread, so every term of A, S and the sum is bounded by that spread, not by
// the depth.  f is a decision of the replay (the first c > 0), so the forward
// and the backward take the same one.
__device__ __forceinline__ float4 dist_payload(float z, uint32_t gid, float kappa) {
  const bool inv = kappa != 0.f;
  return make_float4(z, inv ? kappa / z : 1.f, inv ? 1.f / z : 1.f, __uint_as_float(gid));
}

// k_feat_fwd's walk with (z, q, r, id) as the payload.  kInv: the inverse
// map (the linear one skips the q r factor).  "A contributor so far" is
// A > 0 and "the median is taken" is A >= 0.5, both on the A before the entry:
// no state of their own.
template <bool kInv>
__global__ __launch_bounds__(kWave) void k_dist_fwd(gs_distortion_fwd_args a, float kappa) {
  __shared__ float4 s_rec[kWave * 3];  // per entry: (mx my h00 h11) (ho o - -) (z q r id), h = -q/2
  Replay r;
  const CellGeom cg(a.cam.tile_size);
  const bool any = replay_setup(r, a.cam, a.tiles_x, a.tiles_y, cg.cells(), 0, a.ranges, (uint32_t)a.num_pairs,
                                a.cell_neval, a.live_bits, a.live_words);
  if (r.tile >= a.tiles_x * a.tiles_y) return;
  const int lane = threadIdx.x;
  const uint32_t ngauss = (uint32_t)a.num_gaussians;
  const float4 *recs = reinterpret_cast<const float4 *>(a.records);
  float A = 0.f, S = 0.f, D = 0.f, med_z = 0.f;
  int med_id = -1;
  if (any) {
    const float fx = (float)r.px, fy = (float)r.py;
    float T1 = 1.f, zf = 0.f, rf = 1.f;
    bool run = r.inside;  // A < 0.995 so far; lanes outside the tile or image never run
    float4 n0 = make_float4(0.f, 0.f, 0.f, 0.f), n1 = n0, nf = n0;
    auto fetch = [&](uint32_t wd, unsigned long long m) {
      if ((m >> lane) & 1ull) {
        const uint32_t gid = min(a.sorted_gauss[r.start + 64u * wd + (uint32_t)lane], ngauss - 1u);
        n0 = recs[3 * (size_t)gid];
        n1 = recs[3 * (size_t)gid + 1];
        nf = dist_payload(recs[3 * (size_t)gid + 2].y, gid, kappa);
      }
    };
    unsigned long long mcur = r.live_word(0);
    fetch(0, mcur);
    for (uint32_t wd = 0; wd < r.nwords; ++wd) {
      // (this wave's reads of the previous word precede these writes in its in-order LDS queue)
      if ((mcur >> lane) & 1ull) {
        s_rec[3 * lane] = make_float4(n0.x, n0.y, -0.5f * n0.z, -0.5f * n0.w);
        s_rec[3 * lane + 1] = make_float4(-0.5f * n1.x, n1.y, 0.f, 0.f);
        s_rec[3 * lane + 2] = nf;
      }
      const unsigned long long mnext = wd + 1u < r.nwords ? r.live_word(wd + 1u) : 0ull;
      fetch(wd + 1u, mnext);  // in flight while this word composites
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the staged records, for every lane
      unsigned long long m = mcur;
      while (m) {
        const uint32_t bit = (uint32_t)__builtin_ctzll(m);
        m &= m - 1ull;
        const float4 c0 = s_rec[3 * bit], c1 = s_rec[3 * bit + 1], fv = s_rec[3 * bit + 2];
        const float dx = fx - c0.x, dy = fy - c0.y;
        const float t = conic_s(dx, dy, c0.z, c1.x, c0.w);  // -s/2 (:333)
        const bool lv = run && !(t < kSkipT);                // the :336 skip, decided on s
        const float w = sat01(exp_blend(t));                 // :334
        const float ai = lv ? sat01(c1.y * w) : 0.f;         // :339
        const float c = T1 * ai;                             // :343-344 (T1 = 1 - A)
        // until the first contributor (A == 0) the reference follows the entry: m = 0, and c = +0
        const bool have = A > 0.f;
        zf = have ? zf : fv.x;
        float md = fv.x - zf;
        if constexpr (kInv) {
          rf = have ? rf : fv.z;
          md *= fv.y * rf;
        }
        D = __builtin_fmaf(c, __builtin_fmaf(md, A, -S), D);
        S = __builtin_fmaf(c, md, S);
        if (c > 0.f && A < 0.5f) {  // (A before this entry: the median is not taken yet)
          med_id = (int)__float_as_uint(fv.w);
          med_z = fv.x;
        }
        A = A + c;
        T1 = 1.f - A;
        run = run && A < kAlphaStop;                         // the :352 break
      }
      asm volatile("" ::: "memory");
      mcur = mnext;
    }
  }
  if (!r.inside) return;
  const size_t HW = (size_t)a.cam.image_width * a.cam.image_height;
  const size_t p = (size_t)r.py * a.cam.image_width + r.px;
  a.distortion[p] = 2.f * D;
  a.moments[p] = A;
  a.moments[HW + p] = S;
  a.median_depth[p] = med_z;
  a.median_id[p] = med_id;
}

__global__ __launch_bounds__(kBlock) void k_dist_empty(gs_distortion_fwd_args a, long long pixels) {
  const long long p = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (p < pixels) {
    a.distortion[p] = 0.f;
    a.moments[p] = 0.f;
    a.moments[pixels + p] = 0.f;
    a.median_depth[p] = 0.f;
    a.median_id[p] = -1;
  }
}

// k_feat_bwd's two phases with a per-pixel, per-entry X_i in place of the
// payload's dot product, for a cotangent g on the distortion:
//   X_i = 2 g [m_i (A_{i-1} + A_i - A_n) + S_n - S_i - S_{i-1}]   (= g dD/dc_i),  K = 2 g D
//   dL/dm_i = 2 g c_i (A_{i-1} + A_i - A_n),  dL/dz_i = dL/dm_i q_i r_i   (1 | kappa / z_i^2)
// dL/dm_i depends on the pixel, so phase A hands phase B a third value per
// (entry, pixel) beside (dop, +-c).  Nothing flows through the reference
// depth: sum_i dL/dm_i = 0.
template <bool kInv>
__global__ __launch_bounds__(kWave) void k_dist_bwd(gs_distortion_bwd_args a, float kappa) {
  __shared__ float2 s_dc[kBwdGroup][kBwdRow];  // per group entry and pixel: (dop, c)
  __shared__ float s_dm[kBwdGroup][kBwdRow];   // ... and dL/dm
  __shared__ float2 s_wrec[kBwdGroup * 6];     // the group's records: (mx my h00 h11) (ho o z q) (r - slot -)
  Replay r;
  const int ncell = a.cell_count;
  if (!replay_setup(r, a.cam, a.tiles_x, a.tiles_y, ncell, a.cell_begin, a.ranges, (uint32_t)a.num_pairs,
                    a.cell_neval, a.live_bits, a.live_words))
    return;
  const int qb = r.quad - a.cell_begin;  // the cell's partial group
  const int lane = threadIdx.x;
  const uint32_t ngauss = (uint32_t)a.num_gaussians;
  const float4 *recs = reinterpret_cast<const float4 *>(a.records);
  // the pixel's cotangent and the forward's state (lanes outside read pixel 0, unused)
  const size_t HW = (size_t)a.cam.image_width * a.cam.image_height;
  const size_t p = r.inside ? (size_t)r.py * a.cam.image_width + r.px : 0;
  const float g2 = r.inside ? 2.f * a.g_distortion[p] : 0.f;
  const float An = a.moments[p], Sn = a.moments[HW + p];
  const float fx = (float)r.px, fy = (float)r.py;
  // PG = P - K as one running sum (k_feat_bwd), K = 2 g D
  float PG = -(g2 * a.distortion[p]);
  float A = 0.f, S = 0.f, T1 = 1.f, zf = 0.f, rf = 1.f;
  bool run = r.inside;
  float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, rz = r0;
  auto fetch = [&](uint32_t wd, unsigned long long m) {
    if ((m >> lane) & 1ull) {
      const uint32_t gid = min(a.sorted_gauss[r.start + 64u * wd + (uint32_t)lane], ngauss - 1u);
      r0 = recs[3 * (size_t)gid];
      r1 = recs[3 * (size_t)gid + 1];
      r2 = recs[3 * (size_t)gid + 2];
      rz = dist_payload(r2.y, gid, kappa);
    }
  };
  // Phase B over a group: its k live entries, staged at s_wrec positions 0 .. k - 1.
  auto phase_b = [&](int k) {
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the group buffer rows this wave wrote
    const int j = lane / kBwdLanes, col = lane % kBwdLanes;
    if (j < k) {
      const uint32_t e = (uint32_t)j;
      const float4 ia = reinterpret_cast<const float4 *>(s_wrec)[3 * e];  // mx my h00 h11 (h = -q/2)
      const float4 ib = reinterpret_cast<const float4 *>(s_wrec)[3 * e + 1];  // ho o z q
      const float q00 = -2.f * ia.z, q11 = -2.f * ia.w, qo = -2.f * ib.x;  // (exact)
      const float zr = s_wrec[6 * e + 4].x;
      const uint32_t slot = __float_as_uint(s_wrec[6 * e + 5].x);
      const float hop = -0.5f * ib.y;
      // (k_feat_bwd's column walk: the row moments about the column row nearest the mean)
      const float bx = (float)(r.x0 + col) - ia.x;
      const float rc = __builtin_amdgcn_fmed3f(__builtin_rintf(ia.y - (float)r.y0), 0.f, (float)(kBwdGroup - 1));
      float S0 = 0.f, Soy = 0.f, Soyy = 0.f, g5 = 0.f, g9 = 0.f;
#pragma unroll
      for (int row = 0; row < kBwdGroup; ++row) {
        const int pp = col + 8 * row;  // phase A's lane of that pixel
        const float2 dc = s_dc[j][pp];
        const float dop = dc.x, cs = dc.y;
        const float ds = cs > 0.f ? dop : 0.f;
        const float wr = (float)row - rc;  // exact: small integers
        S0 += ds;
        Soy = __builtin_fmaf(ds, wr, Soy);
        Soyy = __builtin_fmaf(ds, wr * wr, Soyy);
        g5 += dop;
        g9 += s_dm[j][pp];
      }
      S0 *= hop;
      Soy *= hop;
      Soyy *= hop;
      const float by = (float)r.y0 + rc - ia.y;
      float Sx = bx * S0, Sy = __builtin_fmaf(by, S0, Soy);
      float g2s = bx * Sx, g3 = bx * Sy;
      float g4 = __builtin_fmaf(by, __builtin_fmaf(by, S0, 2.f * Soy), Soyy);
      Sx = oct_sum(Sx); Sy = oct_sum(Sy); g2s = oct_sum(g2s); g3 = oct_sum(g3); g4 = oct_sum(g4);
      g5 = oct_sum(g5); g9 = oct_sum(g9);
      if (col == 0) {
        const float g0 = -(2.f * q00 * Sx + qo * Sy), g1 = -(qo * Sx + 2.f * q11 * Sy);
        const size_t sq = (size_t)slot * (uint32_t)ncell + (uint32_t)qb;
        if (slot < (uint32_t)a.num_pairs) {  // (a slot of this frame's T; a corrupt record writes nothing)
          float *out = a.pair_grads + sq * GS_PARTIAL_STRIDE;  // (dense 40-B partials, 8-B aligned: f4_u8)
          *reinterpret_cast<f4_u8 *>(out) = f4_u8{g0, g1, g2s, g3};
          *reinterpret_cast<f4_u8 *>(out + 4) = f4_u8{g4, g5, 0.f, 0.f};
          *reinterpret_cast<f2_u8 *>(out + 8) = f2_u8{0.f, kInv ? g9 * (ib.w * zr) : g9};  // dm/dz = q r
          a.slot_live[sq] = 1;
        }
      }
    }
  };
  unsigned long long mcur = r.live_word(0);
  fetch(0, mcur);
  for (uint32_t wd = 0; wd < r.nwords; ++wd) {
    // the entry's gradient slot, as k_feat_bwd forms it
    const bool mine = (mcur >> lane) & 1ull;
    const uint32_t info = __float_as_uint(r2.w);
    const uint32_t slot = __float_as_uint(r2.z) + (r.ty - ((info >> 12) & 0xFFFu)) * ((info >> 24) + 1u) +
                          (r.tx - (info & 0xFFFu));
    const uint32_t rank =
        __builtin_amdgcn_mbcnt_hi((uint32_t)(mcur >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mcur, 0u));
    const float4 c0 = make_float4(r0.x, r0.y, -0.5f * r0.z, -0.5f * r0.w);
    const float4 c1 = make_float4(-0.5f * r1.x, r1.y, rz.x, rz.y);
    const float4 c2 = make_float4(rz.z, 0.f, __uint_as_float(slot), 0.f);
    const unsigned long long mnext = wd + 1u < r.nwords ? r.live_word(wd + 1u) : 0ull;
    fetch(wd + 1u, mnext);  // in flight while this word replays
    unsigned long long m = mcur;
    uint32_t kb = 0;  // packed position of the group's first entry
    while (m) {
      int k = 0;
      // (the previous group's reads came before these writes in this wave's in-order LDS queue)
      if (mine && rank - kb < (uint32_t)kBwdGroup) {
        float4 *d = reinterpret_cast<float4 *>(&s_wrec[6 * (rank - kb)]);
        d[0] = c0;
        d[1] = c1;
        d[2] = c2;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the staged records, for every lane
      const char *cb = reinterpret_cast<const char *>(s_wrec);
#pragma unroll
      for (int kk = 0; kk < kBwdGroup; ++kk) {
        if (kk > 0 && !m) break;
        m &= m - 1ull;
        const float4 r0v = reinterpret_cast<const float4 *>(cb + 48 * kk)[0];
        const float4 r1v = reinterpret_cast<const float4 *>(cb + 48 * kk)[1];
        const float zr = reinterpret_cast<const float2 *>(cb + 48 * kk)[4].x;
        const float dx = fx - r0v.x, dy = fy - r0v.y;
        const float tq = conic_s(dx, dy, r0v.z, r1v.x, r0v.w);  // -s/2, as in the forward
        const bool live = run && !(tq < kSkipT);
        const float e = exp_blend(tq);
        const float w = sat01(e);
        const float u = r1v.y * w;
        const float ai = sat01(u);
        const float trans = T1;
        const float c = trans * (live ? ai : 0.f);
        // the forward's reference and prefix sums, operation for operation
        const bool have = A > 0.f;
        zf = have ? zf : r1v.z;
        float md = r1v.z - zf;
        if constexpr (kInv) {
          rf = have ? rf : zr;
          md *= r1v.w * rf;
        }
        const float Ap = A, Sp = S;
        S = __builtin_fmaf(c, md, S);
        A = A + c;
        const float u3 = (Ap + A) - An;
        const float X = g2 * __builtin_fmaf(md, u3, (Sn - S) - Sp);
        PG = __builtin_fmaf(c, X, PG);
        const bool term = !(A < kAlphaStop);
        T1 = 1.f - A;
        const float inv = __builtin_amdgcn_rcpf(T1);  // v_rcp_f32 (1 ulp): a gradient factor, no decision
        const float d_live = __builtin_fmaf(inv, PG, X);
        // the terminating contributor has nothing behind it
        const float dal = trans * (term ? X : d_live);
        run = run && !term;
        const float g = (ai == u) ? dal * w : 0.f;
        const float dop = (c > 0.f) ? g : 0.f;
        const float cw = (w == e) ? c : -c;  // c == +0 when skipped
        s_dc[kk][lane] = make_float2(dop, cw);
        s_dm[kk][lane] = (g2 * c) * u3;
        k = kk + 1;
      }
      phase_b(k);
      kb += (uint32_t)k;
    }
    mcur = mnext;
  }
}

// near == far == 0: the linear map (kappa 0); else 0 < near < far, both finite
bool near_far_ok(float near, float far) {
  if (near == 0.f && far == 0.f) return true;
  return near > 0.f && far > near && far <= 3.402823466e+38f;  // (false for NaN)
}

float near_far_kappa(float near, float far) {
  return (near == 0.f && far == 0.f) ? 0.f : (float)((double)far * near / ((double)far - near));
}

int cells_per_tile(int tile_size) {
  const int qx = (tile_size + GS_QUAD - 1) / GS_QUAD;
  return qx * qx;
}

bool tiles_match(const gs_camera &c, int tiles_x, int tiles_y) {
  return tiles_x == (int)div_up(c.image_width, c.tile_size) && tiles_y == (int)div_up(c.image_height, c.tile_size);
}

bool channels_ok(int channels) { return channels >= 1 && channels <= GS_MAX_FEATURE_CHANNELS; }

}  // namespace

// ============================================================ C ABI =======
extern "C" {

gs_status gs_blend_features_forward(const gs_feature_fwd_args *a, gs_stream_t stream) {
  const char *me = "gs_blend_features_forward";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", me);
  if (!cam_ok(a->cam)) return gs_internal_fail(GS_ERR_UNSUPPORTED, kCamMsg, me);
  if (!tiles_match(a->cam, a->tiles_x, a->tiles_y))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: tiles_x/tiles_y do not match the image", me);
  if (!channels_ok(a->channels))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: channels must be in [1, GS_MAX_FEATURE_CHANNELS]", me);
  if (!a->ranges || !a->records || !a->cell_neval || !a->features || !a->out || (a->live_bits && a->live_words <= 0) ||
      (a->num_pairs > 0 && !a->sorted_gauss))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", me);
  if (a->num_pairs < 0 || a->num_gaussians < 1)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative num_pairs or no Gaussians", me);
  const long long chunks = div_up(a->channels, GS_FEATURE_CHUNK);
  const long long blocks = (long long)div_up((long long)a->tiles_x * a->tiles_y, 8) * 8LL * cells_per_tile(a->cam.tile_size);
  // (a launch's work-items, workgroups x 64, must stay below 2^32)
  if (blocks * chunks * kWave > 0xffffffffLL) return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: too many tiles", me);
  k_feat_fwd<<<dim3((unsigned)blocks, (unsigned)chunks), kWave, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(me);
}

gs_status gs_blend_features_backward(const gs_feature_bwd_args *a, gs_stream_t stream) {
  const char *me = "gs_blend_features_backward";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", me);
  if (!cam_ok(a->cam)) return gs_internal_fail(GS_ERR_UNSUPPORTED, kCamMsg, me);
  if (!tiles_match(a->cam, a->tiles_x, a->tiles_y))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: tiles_x/tiles_y do not match the image", me);
  if (!channels_ok(a->channels))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: channels must be in [1, GS_MAX_FEATURE_CHANNELS]", me);
  if (a->chunk < 0 || a->chunk >= (int)div_up(a->channels, GS_FEATURE_CHUNK))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: chunk must be in [0, ceil(channels / 4))", me);
  if (!a->ranges || !a->sorted_gauss || !a->records || !a->cell_neval || !a->features || !a->out || !a->g_out ||
      !a->pair_grads || !a->slot_live || (a->live_bits && a->live_words <= 0))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", me);
  if (a->num_pairs < 0 || a->num_gaussians < 1)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative num_pairs or no Gaussians", me);
  const int cells = cells_per_tile(a->cam.tile_size);
  gs_feature_bwd_args b = *a;
  if (b.cell_count == 0 && b.cell_begin == 0) b.cell_count = cells;  // (0: every cell, one batch)
  if (b.cell_begin < 0 || b.cell_count < 1 || b.cell_begin + b.cell_count > cells)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: the cell batch [cell_begin, cell_begin + cell_count) must lie in "
                "[0, gs_tile_quads(tile_size))", me);
  const long long blocks = (long long)div_up((long long)b.tiles_x * b.tiles_y, 8) * 8LL * b.cell_count;
  if (blocks * kWave > 0xffffffffLL) return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: too many tiles", me);
  k_feat_bwd<<<(unsigned)blocks, kWave, 0, (hipStream_t)stream>>>(b);
  return gs_internal_check_launch(me);
}

gs_status gs_gather_feature_partials(const gs_feature_gather_args *a, gs_stream_t stream) {
  const char *me = "gs_gather_feature_partials";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", me);
  if (a->n < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative n", me);
  if (!a->vis || !a->rects || !a->pair_offset || !a->pair_grads || !a->slot_live || !a->grad_sums || !a->d_features)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", me);
  if (a->partial_groups < 1) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: partial_groups < 1", me);
  if (a->channel_count < 1 || a->channel_count > GS_FEATURE_CHUNK || a->channel_begin < 0 ||
      a->channel_begin + a->channel_count > GS_MAX_FEATURE_CHANNELS ||
      a->d_features_stride < a->channel_begin + a->channel_count)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: channels [channel_begin, channel_begin + channel_count) must be "
                "1..4 columns inside a d_features row", me);
  if (a->n == 0) return GS_OK;
  hipStream_t s = (hipStream_t)stream;
  // (k_gather_slots' lanes per Gaussian for the same partial_groups)
  if (a->partial_groups == 1)
    k_gather_feat<1, 4><<<div_up(4LL * a->n, kBlock), kBlock, 0, s>>>(*a);
  else if (a->partial_groups == 2)
    k_gather_feat<2, 2><<<div_up(4LL * a->n, kBlock), kBlock, 0, s>>>(*a);
  else
    k_gather_feat<4, 2><<<div_up(8LL * a->n, kBlock), kBlock, 0, s>>>(*a);
  return gs_internal_check_launch(me);
}

gs_status gs_blend_contributions(const gs_contrib_args *a, gs_stream_t stream) {
  const char *me = "gs_blend_contributions";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", me);
  if (!cam_ok(a->cam)) return gs_internal_fail(GS_ERR_UNSUPPORTED, kCamMsg, me);
  if (!tiles_match(a->cam, a->tiles_x, a->tiles_y))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: tiles_x/tiles_y do not match the image", me);
  if (a->num_pairs < 0 || a->num_gaussians < 0)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative num_pairs or num_gaussians", me);
  if (!a->ranges || !a->records || !a->cell_neval || !a->partials || !a->slot_live ||
      (a->live_bits && a->live_words <= 0) || (a->num_pairs > 0 && !a->sorted_gauss))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", me);
  if (!a->dominant_id != !a->dominant_weight)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: dominant_id and dominant_weight go together", me);
  const int cells = cells_per_tile(a->cam.tile_size);
  gs_contrib_args b = *a;
  if (b.cell_count == 0 && b.cell_begin == 0) b.cell_count = cells;  // (0: every cell, one batch)
  if (b.cell_begin < 0 || b.cell_count < 1 || b.cell_begin + b.cell_count > cells)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: the cell batch [cell_begin, cell_begin + cell_count) must lie in "
                "[0, gs_tile_quads(tile_size))", me);
  const long long blocks = (long long)div_up((long long)b.tiles_x * b.tiles_y, 8) * 8LL * b.cell_count;
  if (blocks * kWave > 0xffffffffLL) return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: too many tiles", me);
  if (b.num_gaussians == 0 || b.num_pairs == 0) {
    if (!b.dominant_id) return GS_OK;
    const long long pixels = (long long)b.cam.image_width * b.cam.image_height;
    k_contrib_empty<<<div_up(pixels, kBlock), kBlock, 0, (hipStream_t)stream>>>(b.dominant_id, b.dominant_weight, pixels);
    return gs_internal_check_launch(me);
  }
  k_contrib<<<(unsigned)blocks, kWave, 0, (hipStream_t)stream>>>(b);
  return gs_internal_check_launch(me);
}

gs_status gs_blend_distortion_forward(const gs_distortion_fwd_args *a, gs_stream_t stream) {
  const char *me = "gs_blend_distortion_forward";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", me);
  if (!near_far_ok(a->near, a->far))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: near / far must both be 0 (linear depth) or finite with 0 < near < far", me);
  if (!a->ranges || !a->records || !a->cell_neval || !a->distortion || !a->moments || !a->median_depth ||
      !a->median_id || (a->live_bits && a->live_words <= 0) || (a->num_pairs > 0 && !a->sorted_gauss))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", me);
  if (a->num_pairs < 0 || a->num_gaussians < 0)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative num_pairs or num_gaussians", me);
  if (!cam_ok(a->cam)) return gs_internal_fail(GS_ERR_UNSUPPORTED, kCamMsg, me);
  if (!tiles_match(a->cam, a->tiles_x, a->tiles_y))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: tiles_x/tiles_y do not match the image", me);
  const long long blocks = (long long)div_up((long long)a->tiles_x * a->tiles_y, 8) * 8LL * cells_per_tile(a->cam.tile_size);
  // (a launch's work-items, workgroups x 64, must stay below 2^32)
  if (blocks * kWave > 0xffffffffLL) return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: too many tiles", me);
  if (a->num_gaussians == 0 || a->num_pairs == 0) {
    const long long pixels = (long long)a->cam.image_width * a->cam.image_height;
    k_dist_empty<<<div_up(pixels, kBlock), kBlock, 0, (hipStream_t)stream>>>(*a, pixels);
    return gs_internal_check_launch(me);
  }
  const float kappa = near_far_kappa(a->near, a->far);
  if (kappa != 0.f)
    k_dist_fwd<true><<<(unsigned)blocks, kWave, 0, (hipStream_t)stream>>>(*a, kappa);
  else
    k_dist_fwd<false><<<(unsigned)blocks, kWave, 0, (hipStream_t)stream>>>(*a, 0.f);
  return gs_internal_check_launch(me);
}

gs_status gs_blend_distortion_backward(const gs_distortion_bwd_args *a, gs_stream_t stream) {
  const char *me = "gs_blend_distortion_backward";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", me);
  if (!near_far_ok(a->near, a->far))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: near / far must both be 0 (linear depth) or finite with 0 < near < far", me);
  if (!a->ranges || !a->sorted_gauss || !a->records || !a->cell_neval || !a->distortion || !a->moments ||
      !a->g_distortion || !a->pair_grads || !a->slot_live || (a->live_bits && a->live_words <= 0))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", me);
  if (a->num_pairs < 0 || a->num_gaussians < 1)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative num_pairs or no Gaussians", me);
  if (!cam_ok(a->cam)) return gs_internal_fail(GS_ERR_UNSUPPORTED, kCamMsg, me);
  if (!tiles_match(a->cam, a->tiles_x, a->tiles_y))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: tiles_x/tiles_y do not match the image", me);
  const int cells = cells_per_tile(a->cam.tile_size);
  gs_distortion_bwd_args b = *a;
  if (b.cell_count == 0 && b.cell_begin == 0) b.cell_count = cells;  // (0: every cell, one batch)
  if (b.cell_begin < 0 || b.cell_count < 1 || b.cell_begin + b.cell_count > cells)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: the cell batch [cell_begin, cell_begin + cell_count) must lie in "
                "[0, gs_tile_quads(tile_size))", me);
  const long long blocks = (long long)div_up((long long)b.tiles_x * b.tiles_y, 8) * 8LL * b.cell_count;
  if (blocks * kWave > 0xffffffffLL) return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: too many tiles", me);
  const float kappa = near_far_kappa(b.near, b.far);
  if (kappa != 0.f)
    k_dist_bwd<true><<<(unsigned)blocks, kWave, 0, (hipStream_t)stream>>>(b, kappa);
  else
    k_dist_bwd<false><<<(unsigned)blocks, kWave, 0, (hipStream_t)stream>>>(b, 0.f);
  return gs_internal_check_launch(me);
}

gs_status gs_contrib_accumulate(const gs_contrib_gather_args *a, gs_stream_t stream) {
  const char *me = "gs_contrib_accumulate";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", me);
  if (a->n < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative n", me);
  if (!a->vis || !a->rects || !a->pair_offset || !a->partials || !a->slot_live || !a->weight_sum || !a->weight_max ||
      !a->pixels || !a->views)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", me);
  if (a->partial_groups < 1) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: partial_groups < 1", me);
  if (a->n == 0) return GS_OK;
  hipStream_t s = (hipStream_t)stream;
  // (k_gather_slots' lanes per Gaussian for the same partial_groups)
  if (a->partial_groups == 1)
    k_contrib_gather<1, 4><<<div_up(4LL * a->n, kBlock), kBlock, 0, s>>>(*a);
  else if (a->partial_groups == 2)
    k_contrib_gather<2, 2><<<div_up(4LL * a->n, kBlock), kBlock, 0, s>>>(*a);
  else
    k_contrib_gather<4, 2><<<div_up(8LL * a->n, kBlock), kBlock, 0, s>>>(*a);
  return gs_internal_check_launch(me);
}

}  // extern "C"
