// gs_gather_device.h -- the one walk of the per-Gaussian partial gathers
// (k_gather_slots and k_gather_abs of gs_project.hip, k_gather_feat and
// k_contrib_gather of gs_features.hip) and their one host dispatch.
// QL x HL lanes per Gaussian: lane (h, q) of g, at t % (QL HL), walks g's
// slots h, h + HL, h + 2 HL, ... of [pair_offset[g], pair_offset[g] + touches)
// and, of each slot's ng partial groups, adds the groups q, q + QL, ... that
// slot_live flags (groups outer, slots inner); the lane sums are then added
// in lanes_sum's fixed DPP order -- bitwise reproducible, and the same order
// in all four kernels by construction (tests/test_gather_partials.py holds a
// numpy statement of it).  The q lanes of a slot read its partials together,
// and consecutive Gaussians' slots are adjacent (index-order slots):
// coalesced.  Latency decides every one of them: what differs between the
// kernels is the partial, what is added, and how many slots a lane requests
// per round trip.  Not part of the C ABI.
#pragma once
#include <type_traits>

#include "gs_internal.h"
#include "gs_device.h"

namespace {

constexpr int kGatherHL1 = 4;  // slot lanes per Gaussian with one partial group per slot

// Slots per lane per round trip: 3 (k_gather_slots: 56 VGPRs, 8 waves per
// SIMD) against 4 (71, 7 waves): 110.9 -> 105.9 us at C3
// (profiles/r05/gather_nb_ab/); the lane's slot order, and so every sum, is
// the same for any batch size.
#ifndef GS_GATHER_NB
#define GS_GATHER_NB 3
#endif
constexpr int kGatherNB = GS_GATHER_NB;

// The slot lists a gather walks (the public argument structs' shared head)
struct SlotLists {
  int n;
  const uint8_t *vis;
  const uint32_t *rects, *pair_offset;
  const uint8_t *slot_live;  // [T, ng]
  int ng;                    // partial groups per slot
};
template <typename Args>
__host__ __device__ __forceinline__ SlotLists slot_lists(const Args &a) {
  return {a.n, a.vis, a.rects, a.pair_offset, a.slot_live, a.partial_groups};
}

// Lane t's place in Gaussian g's walk: its slot lane h and group lane q, g's
// first slot and slot count (0 for an invisible or out-of-range g).
struct SlotLane {
  int h, q;
  bool valid, seen;  // g < n; and visible
  size_t off;
  uint32_t cnt;
};
template <int QL, int HL>
__device__ __forceinline__ SlotLane slot_lane(const SlotLists &s, long long t, int g) {
  constexpr int LPG = QL * HL;
  static_assert(LPG == 2 || LPG == 4 || LPG == 8, "lanes per Gaussian");
  SlotLane l;
  l.h = (int)((t % LPG) / QL);
  l.q = (int)(t % QL);
  // vis, rect and first slot in one round trip (the empty asm keeps the
  // slot load beside the others: used only under the branch, the compiler
  // would issue it after the vis test, a second round trip)
  l.valid = g < s.n;
  const uint32_t gi = l.valid ? (uint32_t)g : 0u;
  const uint32_t visb = s.vis[gi];
  const uint2 rect = reinterpret_cast<const uint2 *>(s.rects)[gi];
  uint32_t off32 = s.pair_offset[gi];
  asm volatile("" : "+v"(off32));
  l.seen = l.valid && visb;
  l.off = off32;
  l.cnt = l.seen ? rect_touches(rect) : 0u;
  return l;
}

// When a batch's partials are requested:
//   kLoadLazy   after the batch's flags, the live ones only (two round trips
//               per NB x HL slots of g; with NB = 1, "if (!flag) continue")
//   kLoadEager  with the flags, all of them (one round trip; past the end the
//               clamped index re-reads slot e0, and a dead partial is read --
//               whatever the buffer holds -- and never used), masked after
enum : int { kLoadLazy = 0, kLoadEager = 1 };

// The walk of lane l: add(load(i)) for every live (slot, group) of the lane,
// i = slot * ng + group, in the order above; load(i) returns the partial at i
// (a value type; {} when not loaded).
template <int QL, int HL, int NB, int kLoad, typename Load, typename Add>
__device__ __forceinline__ void slot_walk(const SlotLists &s, const SlotLane &l, Load load, Add add) {
  using Partial = decltype(load((size_t)0));
  const uint32_t cnt = l.cnt, ng = (uint32_t)s.ng;
  // lane q sums partial groups q, q + QL, ... of a slot's ng (one pass when ng <= QL)
  for (uint32_t qc = (uint32_t)l.q; cnt > (uint32_t)l.h && qc < ng; qc += QL) {
    const size_t first = l.off * ng + qc;  // (slot e, group qc) at first + ng e
    const uint8_t *flag = s.slot_live + first;
    for (uint32_t e0 = (uint32_t)l.h; e0 < cnt; e0 += NB * HL) {
      // the batch's flags in one round trip, at clamped indices, masked after
      uint32_t f[NB];
      Partial v[NB];
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        const uint32_t e = e0 + HL * i;
        const size_t at = (size_t)ng * (e < cnt ? e : e0);
        f[i] = flag[at];
        if constexpr (kLoad == kLoadEager) v[i] = load(first + at);
      }
      uint32_t fm = 0;
#pragma unroll
      for (int i = 0; i < NB; ++i) fm |= (e0 + HL * i < cnt && f[i]) ? 1u << i : 0u;
      if constexpr (kLoad == kLoadLazy) {
        // all the batch's flags tested before any partial is requested: the partial
        // loads are conditional, so a wait for a later flag placed between them
        // would have to count them out conservatively and drain them
        asm volatile("" : "+v"(fm));
#pragma unroll
        for (int i = 0; i < NB; ++i)
          v[i] = ((fm >> i) & 1u) ? load(first + (size_t)(e0 + HL * i) * ng) : Partial{};
      }
#pragma unroll
      for (int i = 0; i < NB; ++i) {
        if (!((fm >> i) & 1u)) continue;
        add(v[i]);
      }
    }
  }
}

// The dense 40-B gradient partial (8-B aligned: f4_u8) of k_gather_slots and
// k_gather_feat, and its addition to ten sums
struct Partial10 {
  f4_u8 a, b;
  f2_u8 c;
};
__device__ __forceinline__ Partial10 load_partial10(const float *pair_grads, size_t i) {
  const float *src = pair_grads + i * GS_PARTIAL_STRIDE;
  // (non-temporal loads, for data read once, measured +10 us: profiles/r03/experiments.md)
  return {*reinterpret_cast<const f4_u8 *>(src), *reinterpret_cast<const f4_u8 *>(src + 4),
          *reinterpret_cast<const f2_u8 *>(src + 8)};
}
__device__ __forceinline__ void add_partial10(float acc[GS_PAIR_GRAD_FLOATS], const Partial10 &v) {
  acc[0] += v.a.x; acc[1] += v.a.y; acc[2] += v.a.z; acc[3] += v.a.w;
  acc[4] += v.b.x; acc[5] += v.b.y; acc[6] += v.b.z; acc[7] += v.b.w;
  acc[8] += v.c.x; acc[9] += v.c.y;
}

// ---------------------------------------------------------------- host ----
// The slot lists' pointers, the entry point's own buffers (`rest`: all there)
// and partial_groups >= 1
inline gs_status slot_lists_check(const SlotLists &s, bool rest, const char *me) {
  if (!s.vis || !s.rects || !s.pair_offset || !s.slot_live || !rest || s.ng < 1)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null buffer or partial_groups < 1", me);
  return GS_OK;
}

// The lanes per Gaussian <QL, HL> and the grid for a slot's partial groups:
// launch(integral_constant QL, integral_constant HL, blocks)
template <typename Launch>
void gather_dispatch(const SlotLists &s, Launch launch) {
  using std::integral_constant;
  if (s.ng == 1)
    launch(integral_constant<int, 1>{}, integral_constant<int, kGatherHL1>{}, div_up((long long)kGatherHL1 * s.n, kBlock));
  else if (s.ng == 2)
    launch(integral_constant<int, 2>{}, integral_constant<int, 2>{}, div_up(4LL * s.n, kBlock));
  else
    launch(integral_constant<int, 4>{}, integral_constant<int, 2>{}, div_up(8LL * s.n, kBlock));
}

}  // namespace
