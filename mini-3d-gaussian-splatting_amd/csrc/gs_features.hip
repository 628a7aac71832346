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
// k_blend_bwd replays it with.  Everything that forms a decision (exp_blend,
// conic_s, the -Q/2 staging, the s skip, the weight, A = A + c, T1 = 1 - A,
// the stop) is gs_blend_device.h's one copy, which gs_blend.hip is built from
// too, with the same flags (no contraction): the same source gives the same
// bits.  Two walks own the rest of a replay -- word_walk for the forward-type
// passes, group_walk for those that reduce per entry -- so a pass states its
// payload, its accumulation and its stores, and nothing of the decision.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "gsplat_mi355x.h"
#include "gs_internal.h"
#include "gs_device.h"
#include "gs_blend_device.h"
#include "gs_gather_device.h"

namespace {

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

// The replay of this workgroup's cell, one of the ncell cells from cell0 of
// its tile, over the forward's state in f.  false: nothing to replay (a
// padding workgroup is reported through r.tile)
__device__ __forceinline__ bool replay_setup(Replay &r, const gs_replay_frame &f, int ncell, int cell0) {
  const CellGeom cg(f.cam.tile_size);
  const uint32_t T = (uint32_t)f.num_pairs;
  int qb;
  uint32_t end;
  cell_tile(blockIdx.x, ncell, f.ranges, f.tiles_x * f.tiles_y, T, r.tile, qb, r.start, end);
  r.wstop = r.nwords = 0u;
  r.inside = false;
  r.lw = nullptr;
  if (r.tile >= f.tiles_x * f.tiles_y) return false;
  r.quad = cell0 + qb;
  const int lane = threadIdx.x;
  r.tx = (uint32_t)(r.tile % f.tiles_x);
  r.ty = (uint32_t)(r.tile / f.tiles_x);
  const int cx0 = (r.quad % cg.QX) * 8, cy0 = (r.quad / cg.QX) * 8;  // the cell in its tile
  r.x0 = (int)r.tx * cg.L + cx0;
  r.y0 = (int)r.ty * cg.L + cy0;
  r.px = r.x0 + (lane & 7);
  r.py = r.y0 + (lane >> 3);
  r.inside =
      cx0 + (lane & 7) < cg.L && cy0 + (lane >> 3) < cg.L && r.px < f.cam.image_width && r.py < f.cam.image_height;
  if (r.start >= end) return false;
  // the cell's last evaluated entry (never past the list, whatever the word holds)
  r.wstop = min((uint32_t)__builtin_amdgcn_readfirstlane(f.cell_neval[(size_t)r.tile * cg.cells() + r.quad]),
                end - r.start);
  r.nwords = (r.wstop + 63u) >> 6;
  if (f.live_bits)
    r.lw = reinterpret_cast<const unsigned long long *>(f.live_bits) + (size_t)r.quad * f.live_words + r.start / 64u +
           (uint32_t)r.tile;
  return r.wstop != 0u;
}

// ======================================================== word walk =======
// The walk of the forward-type replays (k_feat_fwd, k_dist_fwd), lane = pixel.
// Per 64-entry word of the cell's liveness bitmap: the live entries' records
// and payloads are gathered lane-parallel (the next word's meanwhile, in
// registers), staged in s_rec (3 float4 per lane) and walked in bit order as
// broadcasts.  The weight is k_blend_fwd's: skips folded in (a skipped pair
// gets ai = 0, hence c = +0), c = (1 - A) ai, A = A + c.  A pass gives
//   payload(gid)        the float4 it carries for Gaussian gid,
//   entry(payload, c, A) its accumulation, A the sum before the entry,
// and gets back the pixel's A after the last one.
template <class Payload, class Entry>
__device__ __forceinline__ float word_walk(const Replay &r, const gs_replay_frame &f, float4 *s_rec, Payload payload,
                                           Entry entry) {
  const int lane = threadIdx.x;
  const uint32_t ngauss = (uint32_t)f.num_gaussians;
  const float4 *recs = reinterpret_cast<const float4 *>(f.records);
  const float fx = (float)r.px, fy = (float)r.py;
  float A = 0.f, T1 = 1.f;
  bool run = r.inside;  // A < 0.995 so far; lanes outside the tile or image never run
  float4 n0 = make_float4(0.f, 0.f, 0.f, 0.f), n1 = n0, nf = n0;
  auto fetch = [&](uint32_t wd, unsigned long long m) {
    if ((m >> lane) & 1ull) {
      const uint32_t gid = min(f.sorted_gauss[r.start + 64u * wd + (uint32_t)lane], ngauss - 1u);
      n0 = recs[3 * (size_t)gid];
      n1 = recs[3 * (size_t)gid + 1];
      nf = payload(gid);
    }
  };
  unsigned long long mcur = r.live_word(0);
  fetch(0, mcur);
  for (uint32_t wd = 0; wd < r.nwords; ++wd) {
    // (this wave's reads of the previous word precede these writes in its in-order LDS queue)
    if ((mcur >> lane) & 1ull) {  // per entry: (mx my h00 h11) (ho o - -) payload, h = -q/2
      const float4 h1 = stage_conic1(n1);
      s_rec[3 * lane] = stage_conic0(n0);
      s_rec[3 * lane + 1] = make_float4(h1.x, h1.y, 0.f, 0.f);
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
      const float c = pair_weight(t, c1.y, T1, run).c;
      entry(fv, c, A);
      const bool go = blend_advance(A, T1, c);
      run = run && go;
    }
    asm volatile("" ::: "memory");
    mcur = mnext;
  }
  return A;
}

// ======================================================= group walk =======
// The walk of the replays that reduce over a cell's pixels per entry
// (k_feat_bwd, k_dist_bwd, k_contrib): k_blend_bwd's two phases without its
// tuning (no simple-entry fast path), per group of up to kBwdGroup live
// entries of a word:
//  A (pixel-parallel), per entry: replay the pixel's chain, and the pass puts
//    what it sums into its group buffers' row kk;
//  B (entry-parallel): lanes 8j..8j+7 sum entry j's 64 pixels -- lane 8j + x
//    takes column x -- and reduce with 3 DPP steps.
constexpr int kBwdGroup = 8;
constexpr int kBwdLanes = kWave / kBwdGroup;
constexpr int kBwdRow = kWave + 8;  // rows padded to 72 float2: no bank conflict between a half's rows

// One entry of a pixel's chain, as phase A gets it
struct ChainStep {
  PairWeight p;   // the weight c and what formed it
  float A0, T0;   // A and the transmittance 1 - A before the entry
  float A1, T1;   // ... and after it
  bool term;      // A1 >= 0.995: nothing behind this entry
};

// The staged record of a group entry: (mx my h00 h11) (ho o . .), h = -q/2,
// then per layout the payload p and the entry's gradient slot.
struct Rec3 {  // (mx my h00 h11) (ho o p0 p1) (p2 p3 slot -)
  static constexpr int kF4 = 3;
  static __device__ __forceinline__ void pack(float4 *c, float4 r0, float4 r1, float4 p, uint32_t slot) {
    const float4 h1 = stage_conic1(r1);
    c[0] = stage_conic0(r0);
    c[1] = make_float4(h1.x, h1.y, p.x, p.y);
    c[2] = make_float4(p.z, p.w, __uint_as_float(slot), 0.f);
  }
  static __device__ __forceinline__ uint32_t slot(const float4 *rec) { return __float_as_uint(rec[2].z); }
};
struct Rec2 {  // (mx my h00 h11) (ho o slot p0)
  static constexpr int kF4 = 2;
  static __device__ __forceinline__ void pack(float4 *c, float4 r0, float4 r1, float4 p, uint32_t slot) {
    const float4 h1 = stage_conic1(r1);
    c[0] = stage_conic0(r0);
    c[1] = make_float4(h1.x, h1.y, __uint_as_float(slot), p.x);
  }
  static __device__ __forceinline__ uint32_t slot(const float4 *rec) { return __float_as_uint(rec[1].z); }
};

// A pass gives the layout Rec of s_wrec (kBwdGroup records) and
//   payload(gid, r2)      the float4 it stages for Gaussian gid (r2: its third record),
//   phase_a(kk, rec, st)  entry kk of the group for this pixel: rec its staged record, st its ChainStep,
//   phase_b(k)            the group's k entries reduced and stored, their records at s_wrec positions 0 .. k - 1.
template <class Rec, class Payload, class PhaseA, class PhaseB>
__device__ __forceinline__ void group_walk(const Replay &r, const gs_replay_frame &f, float4 *s_wrec, Payload payload,
                                           PhaseA phase_a, PhaseB phase_b) {
  const int lane = threadIdx.x;
  const uint32_t ngauss = (uint32_t)f.num_gaussians;
  const float4 *recs = reinterpret_cast<const float4 *>(f.records);
  const float fx = (float)r.px, fy = (float)r.py;
  float A = 0.f, T1 = 1.f;
  // `run` is the forward's "A < 0.995 before this entry", carried from the
  // previous entry's own test; lanes outside the tile or image never run
  bool run = r.inside;
  float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, rp = r0;
  auto fetch = [&](uint32_t wd, unsigned long long m) {
    if ((m >> lane) & 1ull) {
      const uint32_t gid = min(f.sorted_gauss[r.start + 64u * wd + (uint32_t)lane], ngauss - 1u);
      r0 = recs[3 * (size_t)gid];
      r1 = recs[3 * (size_t)gid + 1];
      r2 = recs[3 * (size_t)gid + 2];
      rp = payload(gid, r2);
    }
  };
  unsigned long long mcur = r.live_word(0);
  fetch(0, mcur);
  for (uint32_t wd = 0; wd < r.nwords; ++wd) {
    const bool mine = (mcur >> lane) & 1ull;
    // packed: the live entry of rank k (bit order) at position k of its group
    const uint32_t rank =
        __builtin_amdgcn_mbcnt_hi((uint32_t)(mcur >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mcur, 0u));
    // (the conic staged as -Q/2: phase A computes t = -s/2; phase B undoes it)
    float4 c[Rec::kF4];
    Rec::pack(c, r0, r1, rp, entry_slot(r2, r.tx, r.ty));
    const unsigned long long mnext = wd + 1u < r.nwords ? r.live_word(wd + 1u) : 0ull;
    fetch(wd + 1u, mnext);  // in flight while this word replays
    unsigned long long m = mcur;
    uint32_t kb = 0;  // packed position of the group's first entry
    while (m) {
      int k = 0;
      // stage the group (ranks kb .. kb + kBwdGroup - 1; the previous group's
      // reads came before these writes in this wave's in-order LDS queue)
      if (mine && rank - kb < (uint32_t)kBwdGroup) {
#pragma unroll
        for (int i = 0; i < Rec::kF4; ++i) s_wrec[Rec::kF4 * (rank - kb) + i] = c[i];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the staged records, for every lane
#pragma unroll
      for (int kk = 0; kk < kBwdGroup; ++kk) {
        if (kk > 0 && !m) break;
        m &= m - 1ull;
        const float4 *rec = s_wrec + Rec::kF4 * kk;
        const float4 r0v = rec[0], r1v = rec[1];
        const float dx = fx - r0v.x, dy = fy - r0v.y;
        const float tq = conic_s(dx, dy, r0v.z, r1v.x, r0v.w);  // -s/2, as in the forward
        ChainStep st;
        st.p = pair_weight(tq, r1v.y, T1, run);
        st.A0 = A;
        st.T0 = T1;
        st.term = !blend_advance(A, T1, st.p.c);
        st.A1 = A;
        st.T1 = T1;
        phase_a(kk, rec, st);
        run = run && !st.term;
        k = kk + 1;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // the group buffer rows this wave wrote
      phase_b(k);
      kb += (uint32_t)k;
    }
    mcur = mnext;
  }
}

// dL/dalpha_i = T_i (X_i + (P_i - K) / T_{i+1}) of a chain step, PG = P_i - K
// after it, through the two clamps of the weight: (dop, +-c) for phase B,
// the sign bit of c flagging exp(-s/2) > 1 (the weight clamp then blocks dL/ds).
__device__ __forceinline__ float2 step_grad(const ChainStep &st, float X, float PG) {
  // both arms computed, then a select: no divergent branch per entry
  const float inv = __builtin_amdgcn_rcpf(st.T1);  // v_rcp_f32 (1 ulp): a gradient factor, no decision
  const float d_live = __builtin_fmaf(inv, PG, X);
  // the terminating contributor has nothing behind it
  const float dal = st.T0 * (st.term ? X : d_live);
  // (PairWeight: the clamps pass the gradient where ai == u and w == e)
  const float g = (st.p.ai == st.p.u) ? dal * st.p.w : 0.f;
  const float dop = (st.p.c > 0.f) ? g : 0.f;
  const float cw = (st.p.w == st.p.e) ? st.p.c : -st.p.c;  // c == +0 when skipped
  return make_float2(dop, cw);
}

// Phase B of the two backward replays, Rec3 records and (dop, +-c) in s_dc:
// entry j's geometric sums over this lane's column and the entry's flagged
// 40-B partial {dmu_x, dmu_y, dQ00, dQ01, dQ11, d_opacity, tail(j)}.  The
// pass gives row(j, pp, cw), its own sums over pixel pp (phase A's lane) with
// |c| = cw, and tail(j), components 6 to 9 (called by all the entry's lanes:
// it may oct_sum).
template <class Args, class Row, class Tail>
__device__ __forceinline__ void phase_b_geometry(const Replay &r, const Args &a, const float4 *s_wrec,
                                                 const float2 (*s_dc)[kBwdRow], int k, Row row, Tail tail) {
  const int lane = threadIdx.x;
  const int j = lane / kBwdLanes, col = lane % kBwdLanes;
  if (j < k) {
    const float4 *rec = s_wrec + 3 * j;
    const float4 ia = rec[0];                                    // mx my h00 h11 (h = -q/2)
    const float2 ib = make_float2(rec[1].x, rec[1].y);           // ho o
    const float q00 = -2.f * ia.z, q11 = -2.f * ia.w, qo = -2.f * ib.x;  // (exact)
    const uint32_t slot = Rec3::slot(rec);
    const float hop = -0.5f * ib.y;
    // this lane's pixels (x0 + col, y0 + row): dx = bx, dy = by + (row - rc).
    // The row moments are taken about the column row nearest the mean
    // (clamped), always: about row 0 the dy^2 sum of a Gaussian with
    // sigma_y << 1 px cancels (by^2 S0 + 2 by Soy + Soyy with |by| up to 7
    // for a result of ~sigma_y^2 S0), as k_blend_bwd's comment measures.
    const float bx = (float)(r.x0 + col) - ia.x;
    const float rc = __builtin_amdgcn_fmed3f(__builtin_rintf(ia.y - (float)r.y0), 0.f, (float)(kBwdGroup - 1));
    float S0 = 0.f, Soy = 0.f, Soyy = 0.f, g5 = 0.f;
#pragma unroll
    for (int rw = 0; rw < kBwdGroup; ++rw) {
      const int pp = col + 8 * rw;  // phase A's lane of that pixel
      const float2 dc = s_dc[j][pp];
      const float dop = dc.x, cs = dc.y;
      // dL/ds = hop dop: none where the weight clamp bound (sign bit of c)
      // or the pair was skipped (dop = 0 then)
      const float ds = cs > 0.f ? dop : 0.f;
      const float wr = (float)rw - rc;  // exact: small integers
      S0 += ds;
      Soy = __builtin_fmaf(ds, wr, Soy);
      Soyy = __builtin_fmaf(ds, wr * wr, Soyy);
      g5 += dop;
      row(j, pp, fabsf(cs));
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
    g5 = oct_sum(g5);
    const float4 t = tail(j);
    if (col == 0) {
      // dmu = -(2 q00 Sx + qo Sy, qo Sx + 2 q11 Sy)
      const float g0 = -(2.f * q00 * Sx + qo * Sy), g1 = -(qo * Sx + 2.f * q11 * Sy);
      const size_t sq = (size_t)slot * (uint32_t)a.cell_count + (uint32_t)(r.quad - a.cell_begin);
      if (slot < (uint32_t)a.f.num_pairs) {  // (a slot of this frame's T; a corrupt record writes nothing)
        float *out = a.pair_grads + sq * GS_PARTIAL_STRIDE;  // (dense 40-B partials, 8-B aligned: f4_u8)
        *reinterpret_cast<f4_u8 *>(out) = f4_u8{g0, g1, g2, g3};
        *reinterpret_cast<f4_u8 *>(out + 4) = f4_u8{g4, g5, t.x, t.y};
        *reinterpret_cast<f2_u8 *>(out + 8) = f2_u8{t.z, t.w};
        a.slot_live[sq] = 1;
      }
    }
  }
}

// ====================================================== feature fwd =======
// One 64-lane workgroup per (tile, 8x8 cell) and chunk (grid y): the word
// walk with the chunk's four channels as the payload.
__global__ __launch_bounds__(kWave) void k_feat_fwd(gs_feature_fwd_args a) {
  __shared__ float4 s_rec[kWave * 3];  // per entry: (mx my h00 h11) (ho o - -) (f0 f1 f2 f3), h = -q/2
  Replay r;
  const CellGeom cg(a.f.cam.tile_size);
  const bool any = replay_setup(r, a.f, cg.cells(), 0);
  if (r.tile >= a.f.tiles_x * a.f.tiles_y) return;
  const uint32_t chunk = blockIdx.y;
  const float4 *feat = reinterpret_cast<const float4 *>(a.features) + (size_t)chunk * (uint32_t)a.f.num_gaussians;
  float f0 = 0.f, f1 = 0.f, f2 = 0.f, f3 = 0.f;
  if (any)
    word_walk(
        r, a.f, s_rec, [&](uint32_t gid) { return feat[gid]; },
        [&](const float4 &fv, float c, float) {
          f0 = __builtin_fmaf(c, fv.x, f0);
          f1 = __builtin_fmaf(c, fv.y, f1);
          f2 = __builtin_fmaf(c, fv.z, f2);
          f3 = __builtin_fmaf(c, fv.w, f3);
        });
  if (!r.inside) return;
  const size_t HW = (size_t)a.f.cam.image_width * a.f.cam.image_height;
  const size_t p = (size_t)r.py * a.f.cam.image_width + r.px;
  const uint32_t ch = chunk * GS_FEATURE_CHUNK, C = (uint32_t)a.channels;
  a.out[(size_t)ch * HW + p] = f0;
  if (ch + 1u < C) a.out[(size_t)(ch + 1u) * HW + p] = f1;
  if (ch + 2u < C) a.out[(size_t)(ch + 2u) * HW + p] = f2;
  if (ch + 3u < C) a.out[(size_t)(ch + 3u) * HW + p] = f3;
}

// ====================================================== feature bwd =======
// The group walk over one chunk's payload: phase A puts (dop, c) into the
// group buffer, phase B adds the four channel sums to the geometric ones.
// (At most 6 waves per SIMD, what the kernel ran at with its own loop, 76
// VGPRs: allocated down to 72 for a seventh wave it measured 3 to 9 us slower
// per launch at C3, as k_blend_bwd did at 7.)
__global__ __launch_bounds__(kWave) __attribute__((amdgpu_waves_per_eu(1, 6))) void k_feat_bwd(gs_feature_bwd_args a) {
  __shared__ float2 s_dc[kBwdGroup][kBwdRow];  // per group entry and pixel: (dop, c)
  __shared__ float4 s_pg[kWave];               // per pixel: dL/dout of the chunk's four channels
  __shared__ float2 s_wrec[kBwdGroup * 6];     // the group's records: (mx my h00 h11) (ho o f0 f1) (f2 f3 slot -)
  Replay r;
  if (!replay_setup(r, a.f, a.cell_count, a.cell_begin)) return;
  const int lane = threadIdx.x;
  const float4 *feat = reinterpret_cast<const float4 *>(a.features) + (size_t)a.chunk * (uint32_t)a.f.num_gaussians;
  // the pixel's cotangents and outputs of this chunk (channels past C: zero;
  // lanes outside read pixel 0, unused)
  const size_t HW = (size_t)a.f.cam.image_width * a.f.cam.image_height;
  const size_t p = r.inside ? (size_t)r.py * a.f.cam.image_width + r.px : 0;
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
  // dL/dalpha_i = T_i (X_i + (P_i - K) / T_{i+1}): PG = P - K carried as one
  // running sum (a gradient factor, no decision), P starts at 0 (no background)
  const float K = (gF[0] * oF[0] + gF[1] * oF[1]) + (gF[2] * oF[2] + gF[3] * oF[3]);
  float PG = -K;
  float4 *wrec = reinterpret_cast<float4 *>(s_wrec);
  group_walk<Rec3>(
      r, a.f, wrec, [&](uint32_t gid, const float4 &) { return feat[gid]; },
      [&](int kk, const float4 *rec, const ChainStep &st) {
        const float4 r1v = rec[1];
        const float2 f23 = make_float2(rec[2].x, rec[2].y);
        const float X = __builtin_fmaf(gF[0], r1v.z, __builtin_fmaf(gF[1], r1v.w, __builtin_fmaf(gF[2], f23.x, gF[3] * f23.y)));
        PG = __builtin_fmaf(st.p.c, X, PG);
        s_dc[kk][lane] = step_grad(st, X, PG);
      },
      [&](int k) {
        float g6 = 0.f, g7 = 0.f, g8 = 0.f, g9 = 0.f;
        phase_b_geometry(
            r, a, wrec, s_dc, k,
            [&](int, int pp, float cw) {
              const float4 pg = s_pg[pp];
              g6 = __builtin_fmaf(pg.x, cw, g6);
              g7 = __builtin_fmaf(pg.y, cw, g7);
              g8 = __builtin_fmaf(pg.z, cw, g8);
              g9 = __builtin_fmaf(pg.w, cw, g9);
            },
            [&](int) { return make_float4(oct_sum(g6), oct_sum(g7), oct_sum(g8), oct_sum(g9)); });
      });
}

// ========================================================== gather ========
// slot_walk (gs_gather_device.h) over a chunk's 40-B partials, a slot at a
// time: k_gather_slots' sums, stored as the chunk's.
template <int QL, int HL>
__global__ __launch_bounds__(kBlock) void k_gather_feat(gs_feature_gather_args a) {
  constexpr int LPG = QL * HL;
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int g = (int)(t / LPG);
  const SlotLists s = slot_lists(a);
  const SlotLane l = slot_lane<QL, HL>(s, t, g);
  float acc[GS_PAIR_GRAD_FLOATS];
#pragma unroll
  for (int k = 0; k < GS_PAIR_GRAD_FLOATS; ++k) acc[k] = 0.f;
  slot_walk<QL, HL, 1, kLoadLazy>(
      s, l, [&](size_t i) { return load_partial10(a.pair_grads, i); }, [&](const Partial10 &v) { add_partial10(acc, v); });
#pragma unroll
  for (int k = 0; k < GS_PAIR_GRAD_FLOATS; ++k) acc[k] = lanes_sum<LPG>(acc[k]);
  if ((t % LPG) != 0 || !l.valid) return;
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

__global__ __launch_bounds__(kWave) void k_contrib(gs_contrib_args a) {
  __shared__ float s_c[kBwdGroup][kCtbRow];  // per group entry and pixel: c
  __shared__ float4 s_wrec[kBwdGroup * 2];   // the group's records: (mx my h00 h11) (ho o slot gid)
  Replay r;
  const bool any = replay_setup(r, a.f, a.cell_count, a.cell_begin);
  if (r.tile >= a.f.tiles_x * a.f.tiles_y) return;
  const int lane = threadIdx.x;
  float best = 0.f;
  int best_id = -1;
  if (any)
    group_walk<Rec2>(
        r, a.f, s_wrec, [](uint32_t gid, const float4 &) { return make_float4(__uint_as_float(gid), 0.f, 0.f, 0.f); },
        [&](int kk, const float4 *rec, const ChainStep &st) {
          const float c = st.p.c;
          if (c > best) {
            best = c;
            best_id = (int)__float_as_uint(rec[1].w);
          }
          s_c[kk][lane] = c;
        },
        [&](int k) {
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
            mx = lanes_max<8>(mx);
            cnt = oct_sum(cnt);  // (small integers: exact)
            if (col == 0) {
              const uint32_t slot = Rec2::slot(s_wrec + 2 * j);
              if (slot < (uint32_t)a.f.num_pairs) {  // (a slot of this frame's T; a corrupt record writes nothing)
                const size_t sq = (size_t)slot * (uint32_t)a.cell_count + (uint32_t)(r.quad - a.cell_begin);
                reinterpret_cast<float4 *>(a.partials)[sq] = make_float4(sum, mx, cnt, 0.f);
                a.slot_live[sq] = 1;
              }
            }
          }
        });
  if (a.dominant_id && r.inside) {
    const size_t p = (size_t)r.py * a.f.cam.image_width + r.px;
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

// slot_walk (gs_gather_device.h) over the 16-byte contribution partials, a
// slot at a time; the lane tree of the sums, over max and over integers
template <int QL, int HL>
__global__ __launch_bounds__(kBlock) void k_contrib_gather(gs_contrib_gather_args a) {
  constexpr int LPG = QL * HL;
  const long long t = (long long)blockIdx.x * kBlock + threadIdx.x;
  const int g = (int)(t / LPG);
  const SlotLists sl = slot_lists(a);
  const SlotLane l = slot_lane<QL, HL>(sl, t, g);
  float s = 0.f, m = 0.f;
  int ki = 0;  // (counts as integers: a Gaussian's total may pass 2^24)
  slot_walk<QL, HL, 1, kLoadLazy>(
      sl, l, [&](size_t i) { return reinterpret_cast<const float4 *>(a.partials)[i]; },
      [&](const float4 &v) {
        s += v.x;
        m = fmaxf(m, v.y);
        ki += (int)v.z;
      });
  s = lanes_sum<LPG>(s);
  m = lanes_max<LPG>(m);
  ki = lanes_sum<LPG>(ki);
  if ((t % LPG) != 0 || !l.seen) return;
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

// The word walk with (z, q, r, id) as the payload.  kInv: the inverse map
// (the linear one skips the q r factor).  "A contributor so far" is A > 0 and
// "the median is taken" is A >= 0.5, both on the A before the entry: no state
// of their own.
template <bool kInv>
__global__ __launch_bounds__(kWave) void k_dist_fwd(gs_distortion_fwd_args a, float kappa) {
  __shared__ float4 s_rec[kWave * 3];  // per entry: (mx my h00 h11) (ho o - -) (z q r id), h = -q/2
  Replay r;
  const CellGeom cg(a.f.cam.tile_size);
  const bool any = replay_setup(r, a.f, cg.cells(), 0);
  if (r.tile >= a.f.tiles_x * a.f.tiles_y) return;
  const float4 *recs = reinterpret_cast<const float4 *>(a.f.records);
  float A = 0.f, S = 0.f, D = 0.f, med_z = 0.f, zf = 0.f, rf = 1.f;
  int med_id = -1;
  if (any)
    A = word_walk(
        r, a.f, s_rec, [&](uint32_t gid) { return dist_payload(recs[3 * (size_t)gid + 2].y, gid, kappa); },
        [&](const float4 &fv, float c, float Ap) {
          // until the first contributor (A == 0) the reference follows the entry: m = 0, and c = +0
          const bool have = Ap > 0.f;
          zf = have ? zf : fv.x;
          float md = fv.x - zf;
          if constexpr (kInv) {
            rf = have ? rf : fv.z;
            md *= fv.y * rf;
          }
          D = __builtin_fmaf(c, __builtin_fmaf(md, Ap, -S), D);
          S = __builtin_fmaf(c, md, S);
          if (c > 0.f && Ap < 0.5f) {  // (A before this entry: the median is not taken yet)
            med_id = (int)__float_as_uint(fv.w);
            med_z = fv.x;
          }
        });
  if (!r.inside) return;
  const size_t HW = (size_t)a.f.cam.image_width * a.f.cam.image_height;
  const size_t p = (size_t)r.py * a.f.cam.image_width + r.px;
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

// The group walk with a per-pixel, per-entry X_i in place of the feature
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
  if (!replay_setup(r, a.f, a.cell_count, a.cell_begin)) return;
  const int lane = threadIdx.x;
  // the pixel's cotangent and the forward's state (lanes outside read pixel 0, unused)
  const size_t HW = (size_t)a.f.cam.image_width * a.f.cam.image_height;
  const size_t p = r.inside ? (size_t)r.py * a.f.cam.image_width + r.px : 0;
  const float g2 = r.inside ? 2.f * a.g_distortion[p] : 0.f;
  const float An = a.moments[p], Sn = a.moments[HW + p];
  // PG = P - K as one running sum (k_feat_bwd), K = 2 g D
  float PG = -(g2 * a.distortion[p]);
  float S = 0.f, zf = 0.f, rf = 1.f;
  float4 *wrec = reinterpret_cast<float4 *>(s_wrec);
  group_walk<Rec3>(
      r, a.f, wrec,
      [&](uint32_t gid, const float4 &r2) {
        const float4 zqr = dist_payload(r2.y, gid, kappa);
        return make_float4(zqr.x, zqr.y, zqr.z, 0.f);  // (the id is not staged)
      },
      [&](int kk, const float4 *rec, const ChainStep &st) {
        const float4 r1v = rec[1];
        const float zr = rec[2].x;
        const float c = st.p.c;
        // the forward's reference and prefix sums, operation for operation
        const bool have = st.A0 > 0.f;
        zf = have ? zf : r1v.z;
        float md = r1v.z - zf;
        if constexpr (kInv) {
          rf = have ? rf : zr;
          md *= r1v.w * rf;
        }
        const float Sp = S;
        S = __builtin_fmaf(c, md, S);
        const float u3 = (st.A0 + st.A1) - An;
        const float X = g2 * __builtin_fmaf(md, u3, (Sn - S) - Sp);
        PG = __builtin_fmaf(c, X, PG);
        s_dc[kk][lane] = step_grad(st, X, PG);
        s_dm[kk][lane] = (g2 * c) * u3;
      },
      [&](int k) {
        float g9 = 0.f;
        phase_b_geometry(
            r, a, wrec, s_dc, k, [&](int j, int pp, float) { g9 += s_dm[j][pp]; },
            [&](int j) {
              const float dm = oct_sum(g9);
              const float q = wrec[3 * j + 1].w, zr = wrec[3 * j + 2].x;
              return make_float4(0.f, 0.f, 0.f, kInv ? dm * (q * zr) : dm);  // dm/dz = q r
            });
      });
}

// near == far == 0: the linear map (kappa 0); else 0 < near < far, both finite
bool near_far_ok(float near, float far) {
  if (near == 0.f && far == 0.f) return true;
  return near > 0.f && far > near && far <= 3.402823466e+38f;  // (false for NaN)
}

float near_far_kappa(float near, float far) {
  return (near == 0.f && far == 0.f) ? 0.f : (float)((double)far * near / ((double)far - near));
}

// The fault in a pass's own scalars, as the message it is reported with, or nullptr
const char *channels_fault(int channels, int chunk) {
  if (channels < 1 || channels > GS_MAX_FEATURE_CHANNELS) return "%s: channels must be in [1, GS_MAX_FEATURE_CHANNELS]";
  if (chunk < 0 || chunk >= (int)div_up(channels, GS_FEATURE_CHUNK))
    return "%s: chunk must be in [0, ceil(channels / 4))";
  return nullptr;
}

const char *near_far_fault(float near, float far) {
  if (near_far_ok(near, far)) return nullptr;
  return "%s: near / far must both be 0 (linear depth) or finite with 0 < near < far";
}

// The checks every replay makes of the colour forward's state, in one order:
// the camera, the tile grid, own_fault (the pass's own scalars, above), the
// frame's buffers, the counts.  list_always: the pass reads sorted_gauss
// whatever num_pairs is (the backwards); otherwise only a frame with entries
// needs it.  min_gaussians: 1 for the passes that index rows of a
// per-Gaussian input, 0 for those that accept an empty model.
gs_status replay_frame_check(const gs_replay_frame &f, const char *me, bool list_always, int min_gaussians,
                             const char *own_fault = nullptr) {
  if (!cam_ok(f.cam)) return gs_internal_fail(GS_ERR_UNSUPPORTED, kCamMsg, me);
  if (!tiles_match(f.cam, f.tiles_x, f.tiles_y))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: tiles_x/tiles_y do not match the image", me);
  if (own_fault) return gs_internal_fail(GS_ERR_INVALID_ARG, own_fault, me);
  if (!f.ranges || !f.records || !f.cell_neval || (f.live_bits && f.live_words <= 0) ||
      ((list_always || f.num_pairs > 0) && !f.sorted_gauss))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", me);
  if (f.num_pairs < 0 || f.num_gaussians < min_gaussians)
    return gs_internal_fail(GS_ERR_INVALID_ARG, min_gaussians > 0 ? "%s: negative num_pairs or no Gaussians"
                                                                  : "%s: negative num_pairs or num_gaussians", me);
  return GS_OK;
}

// cell_batch for a replay's arguments b: its cell_begin / cell_count over its frame's tiles
template <class Args>
gs_status replay_cell_batch(Args &b, const char *me, long long *blocks) {
  return cell_batch(b.f.cam.tile_size, b.f.tiles_x, b.f.tiles_y, b.cell_begin, b.cell_count, me, blocks);
}

}  // namespace

// ============================================================ C ABI =======
extern "C" {

gs_status gs_blend_features_forward(const gs_feature_fwd_args *a, gs_stream_t stream) {
  const char *me = "gs_blend_features_forward";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", me);
  if (const gs_status st = replay_frame_check(a->f, me, false, 1, channels_fault(a->channels, 0))) return st;
  if (!a->features || !a->out) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", me);
  const long long chunks = div_up(a->channels, GS_FEATURE_CHUNK);
  long long blocks;
  if (!cell_grid(a->f.tiles_x, a->f.tiles_y, cells_per_tile(a->f.cam.tile_size), &blocks, chunks))
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: too many tiles", me);
  k_feat_fwd<<<dim3((unsigned)blocks, (unsigned)chunks), kWave, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(me);
}

gs_status gs_blend_features_backward(const gs_feature_bwd_args *a, gs_stream_t stream) {
  const char *me = "gs_blend_features_backward";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", me);
  if (const gs_status st = replay_frame_check(a->f, me, true, 1, channels_fault(a->channels, a->chunk))) return st;
  if (!a->features || !a->out || !a->g_out || !a->pair_grads || !a->slot_live)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", me);
  gs_feature_bwd_args b = *a;
  long long blocks;
  if (const gs_status st = replay_cell_batch(b, me, &blocks)) return st;
  k_feat_bwd<<<(unsigned)blocks, kWave, 0, (hipStream_t)stream>>>(b);
  return gs_internal_check_launch(me);
}

gs_status gs_gather_feature_partials(const gs_feature_gather_args *a, gs_stream_t stream) {
  const char *me = "gs_gather_feature_partials";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", me);
  if (a->n < 0) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative n", me);
  if (const gs_status st = slot_lists_check(slot_lists(*a), a->pair_grads && a->grad_sums && a->d_features, me)) return st;
  if (a->channel_count < 1 || a->channel_count > GS_FEATURE_CHUNK || a->channel_begin < 0 ||
      a->channel_begin + a->channel_count > GS_MAX_FEATURE_CHANNELS ||
      a->d_features_stride < a->channel_begin + a->channel_count)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: channels [channel_begin, channel_begin + channel_count) must be "
                "1..4 columns inside a d_features row", me);
  if (a->n == 0) return GS_OK;
  gather_dispatch(slot_lists(*a), [&](auto ql, auto hl, unsigned blocks) {
    k_gather_feat<decltype(ql)::value, decltype(hl)::value><<<blocks, kBlock, 0, (hipStream_t)stream>>>(*a);
  });
  return gs_internal_check_launch(me);
}

gs_status gs_blend_contributions(const gs_contrib_args *a, gs_stream_t stream) {
  const char *me = "gs_blend_contributions";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", me);
  if (const gs_status st = replay_frame_check(a->f, me, false, 0)) return st;
  if (!a->partials || !a->slot_live) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", me);
  if (!a->dominant_id != !a->dominant_weight)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: dominant_id and dominant_weight go together", me);
  gs_contrib_args b = *a;
  long long blocks;
  if (const gs_status st = replay_cell_batch(b, me, &blocks)) return st;
  if (b.f.num_gaussians == 0 || b.f.num_pairs == 0) {
    if (!b.dominant_id) return GS_OK;
    const long long pixels = (long long)b.f.cam.image_width * b.f.cam.image_height;
    k_contrib_empty<<<div_up(pixels, kBlock), kBlock, 0, (hipStream_t)stream>>>(b.dominant_id, b.dominant_weight, pixels);
    return gs_internal_check_launch(me);
  }
  k_contrib<<<(unsigned)blocks, kWave, 0, (hipStream_t)stream>>>(b);
  return gs_internal_check_launch(me);
}

gs_status gs_blend_distortion_forward(const gs_distortion_fwd_args *a, gs_stream_t stream) {
  const char *me = "gs_blend_distortion_forward";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", me);
  if (const gs_status st = replay_frame_check(a->f, me, false, 0, near_far_fault(a->near, a->far))) return st;
  if (!a->distortion || !a->moments || !a->median_depth || !a->median_id)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", me);
  long long blocks;
  if (!cell_grid(a->f.tiles_x, a->f.tiles_y, cells_per_tile(a->f.cam.tile_size), &blocks))
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: too many tiles", me);
  if (a->f.num_gaussians == 0 || a->f.num_pairs == 0) {
    const long long pixels = (long long)a->f.cam.image_width * a->f.cam.image_height;
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
  if (const gs_status st = replay_frame_check(a->f, me, true, 1, near_far_fault(a->near, a->far))) return st;
  if (!a->distortion || !a->moments || !a->g_distortion || !a->pair_grads || !a->slot_live)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer", me);
  gs_distortion_bwd_args b = *a;
  long long blocks;
  if (const gs_status st = replay_cell_batch(b, me, &blocks)) return st;
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
  if (const gs_status st = slot_lists_check(
          slot_lists(*a), a->partials && a->weight_sum && a->weight_max && a->pixels && a->views, me))
    return st;
  if (a->n == 0) return GS_OK;
  gather_dispatch(slot_lists(*a), [&](auto ql, auto hl, unsigned blocks) {
    k_contrib_gather<decltype(ql)::value, decltype(hl)::value><<<blocks, kBlock, 0, (hipStream_t)stream>>>(*a);
  });
  return gs_internal_check_launch(me);
}

}  // extern "C"
