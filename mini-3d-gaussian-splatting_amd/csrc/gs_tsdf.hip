// gs_tsdf.hip -- TSDF fusion of rendered depth maps and surface-nets mesh
// extraction (include/gsplat_mi355x.h, "TSDF fusion and mesh extraction").
//
// No atomics anywhere, the same bits every run.  The fusion runs one thread
// per node with the node in registers over the launch's views; the extraction
// is a classification from an LDS image of side / validity bits and two
// gathers (vertices per active cell, faces per emitting node) placed by the
// caller's prefix sums.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "gs_device.h"
#include "gs_internal.h"
#include "gsplat_mi355x.h"

namespace {

// ------------------------------------------------------------- fusion ----
// One thread owns a node; a wave owns 64 adjacent nodes of a row (256 B of
// every array), a workgroup 64 x 4 x 1 nodes.  Every lane walks the same camera
// rows (uniform addresses: 64 B per view through the scalar cache).  The node
// is loaded at its first update and stored once, after the last view, so a
// node outside every frustum costs no volume traffic at all: 8 B (20 B with
// colour) read and written per updated node and launch, plus the map samples.
//
// The map samples are what the launch costs: a node is about four pixels from
// its neighbour at 256^3 and 1080p, so a wave's gather touches up to 64 lines.
// What decides their hit rate is how much of the maps the workgroups in flight
// cover together, so the workgroups are ordered for that (for speed only; any
// order gives the same bits): rows of blocks form super-tiles of sy x sz
// (32 x 32 nodes in y, z), x fastest inside, and every XCD -- consecutive block
// ids are dealt round-robin over the 8 -- takes a contiguous share of the order,
// so that each L2 serves one compact part of the volume.
constexpr int kIx = 64, kIy = kBlock / kIx;  // the workgroup's nodes in x and y
constexpr int kSy = 8, kSz = 32;             // a super-tile: up to 8 x 32 rows of blocks
constexpr int kXcds = 8;

struct IntegrateOrder {
  int bx, sy, sz, ty;  // blocks in x; the super-tile's block rows in y, z; super-tiles in y
  unsigned blocks;     // the launch: whole super-tiles (a block outside the volume returns at once)
};

template <bool COLOR>
__global__ __launch_bounds__(kBlock) void k_tsdf_integrate(gs_tsdf_integrate_args a, IntegrateOrder o) {
  // this block's place in the order: XCD b % 8 takes the b / 8-th of its contiguous share
  const unsigned q = o.blocks / kXcds, r = o.blocks % kXcds, xcd = blockIdx.x % kXcds;
  const unsigned c = xcd * q + min(xcd, r) + blockIdx.x / kXcds;
  const unsigned per_tile = (unsigned)(o.bx * o.sy * o.sz);
  const unsigned tile = c / per_tile, in = c - tile * per_tile;
  const int ibx = (int)(in % (unsigned)o.bx), rest = (int)(in / (unsigned)o.bx);
  const int i = ibx * kIx + (int)(threadIdx.x & (kIx - 1));
  const int j = ((int)(tile % (unsigned)o.ty) * o.sy + rest % o.sy) * kIy + (int)(threadIdx.x / kIx);
  const int k = (int)(tile / (unsigned)o.ty) * o.sz + rest / o.sy;
  if (i >= a.vol.nx || j >= a.vol.ny || k >= a.vol.nz) return;
  const long long nodes = (long long)a.vol.nx * a.vol.ny * a.vol.nz;
  const long long n = ((long long)k * a.vol.ny + j) * a.vol.nx + i;
  const float h = a.vol.voxel_size;
  const float x = a.vol.origin[0] + h * (float)i, y = a.vol.origin[1] + h * (float)j, z = a.vol.origin[2] + h * (float)k;
  const float fw = (float)a.width, fh = (float)a.height;
  const size_t hw = (size_t)a.width * (size_t)a.height;
  const float *__restrict__ cams = a.cameras;
  bool touched = false;
  float t = 0.f, w = 0.f, c0 = 0.f, c1 = 0.f, c2 = 0.f;
  for (int v = 0; v < a.num_views; ++v) {
    const float *cam = cams + (size_t)v * GS_TSDF_CAMERA_FLOATS;
    const float Z = ((cam[8] * x + cam[9] * y) + cam[10] * z) + cam[11];
    if (!(Z > a.near)) continue;
    const float X = ((cam[0] * x + cam[1] * y) + cam[2] * z) + cam[3];
    const float Y = ((cam[4] * x + cam[5] * y) + cam[6] * z) + cam[7];
    const float px = (cam[12] * X) / Z + cam[14];
    const float py = (-cam[13] * Y) / Z + cam[15];
    const float fu = floorf(px + 0.5f), fv = floorf(py + 0.5f);
    if (!(fu >= 0.f && fu < fw && fv >= 0.f && fv < fh)) continue;  // (a NaN skips)
    const size_t at = (size_t)(int)fv * (size_t)a.width + (size_t)(int)fu;
    const float d = a.depth[(size_t)v * hw + at];
    if (!(d > 0.f)) continue;
    if (d > a.depth_max) continue;
    if (a.alpha && a.alpha[(size_t)v * hw + at] < a.alpha_min) continue;
    const float s = d - Z;
    if (s < -a.trunc) continue;
    const float tau = fminf(1.f, s / a.trunc);
    if (!touched) {
      touched = true;
      t = a.vol.tsdf[n];
      w = a.vol.weight[n];
      if constexpr (COLOR) {
        c0 = a.vol.color[n];
        c1 = a.vol.color[(size_t)nodes + (size_t)n];
        c2 = a.vol.color[2 * (size_t)nodes + (size_t)n];
      }
    }
    const float w1 = w + 1.f;
    t = (t * w + tau) / w1;
    if constexpr (COLOR) {
      const float *img = a.image + (size_t)v * 3 * hw + at;
      c0 = (c0 * w + img[0]) / w1;
      c1 = (c1 * w + img[hw]) / w1;
      c2 = (c2 * w + img[2 * hw]) / w1;
    }
    w = w1;
  }
  if (!touched) return;
  a.vol.tsdf[n] = t;
  a.vol.weight[n] = w;
  if constexpr (COLOR) {
    a.vol.color[n] = c0;
    a.vol.color[(size_t)nodes + (size_t)n] = c1;
    a.vol.color[2 * (size_t)nodes + (size_t)n] = c2;
  }
}

// ----------------------------------------------------------- classify ----
// A workgroup owns a kTx x kTy x kTz tile of nodes.  A node's three edges ask
// for the side of 4 nodes and the validity of 27 (the four cells around each
// edge), a cell for 8 of each: read from memory that is 8 B x 35 a node.  The
// tile's nodes and a one-node apron go into LDS once, as two bits each (8 B x
// 2040 / 1024 = 15.9 B a node from L2, the apron's rows mostly hits), then the
// cells' bits are formed there, then the nodes' masks.  A node that does not
// exist is invalid, so a cell that does not exist is.
constexpr int kTx = 32, kTy = 8, kTz = 4;
constexpr int kHx = kTx + 2, kHy = kTy + 2, kHz = kTz + 2;           // nodes with the apron
constexpr int kCx = kHx - 1, kCy = kHy - 1, kCz = kHz - 1;           // cells anchored at halo nodes
constexpr uint8_t kInside = 1, kOk = 2;                              // node bits
constexpr uint8_t kValid = 1, kActive = 2;                           // cell bits

__global__ __launch_bounds__(kBlock) void k_mesh_classify(gs_mesh_args a) {
  __shared__ uint8_t s_node[kHz][kHy][kHx];
  __shared__ uint8_t s_cell[kCz][kCy][kCx];
  const int nx = a.vol.nx, ny = a.vol.ny, nz = a.vol.nz;
  const int x0 = blockIdx.x * kTx, y0 = blockIdx.y * kTy, z0 = blockIdx.z * kTz;
  for (int e = threadIdx.x; e < kHz * kHy * kHx; e += kBlock) {
    const int hx = e % kHx, hy = (e / kHx) % kHy, hz = e / (kHx * kHy);
    const int gx = x0 - 1 + hx, gy = y0 - 1 + hy, gz = z0 - 1 + hz;
    uint8_t bits = 0;
    if (gx >= 0 && gx < nx && gy >= 0 && gy < ny && gz >= 0 && gz < nz) {
      const size_t at = ((size_t)gz * (size_t)ny + (size_t)gy) * (size_t)nx + (size_t)gx;
      bits = (a.vol.tsdf[at] < 0.f ? kInside : 0) | (a.vol.weight[at] >= a.min_weight ? kOk : 0);
    }
    s_node[hz][hy][hx] = bits;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kCz * kCy * kCx; e += kBlock) {
    const int hx = e % kCx, hy = (e / kCx) % kCy, hz = e / (kCx * kCy);
    int ok = 0, inside = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
      const uint8_t b = s_node[hz + (c >> 2)][hy + ((c >> 1) & 1)][hx + (c & 1)];
      ok += (b & kOk) ? 1 : 0;
      inside += (b & kInside) ? 1 : 0;
    }
    const bool valid = ok == 8, active = valid && inside > 0 && inside < 8;
    s_cell[hz][hy][hx] = (valid ? kValid : 0) | (active ? kActive : 0);
    // the tile's own cells (anchored at its nodes) that exist in the cell grid
    const int gx = x0 - 1 + hx, gy = y0 - 1 + hy, gz = z0 - 1 + hz;
    if (hx >= 1 && hy >= 1 && hz >= 1 && gx < nx - 1 && gy < ny - 1 && gz < nz - 1)
      a.cell_active[((size_t)gz * (size_t)(ny - 1) + (size_t)gy) * (size_t)(nx - 1) + (size_t)gx] = active ? 1 : 0;
  }
  __syncthreads();
  for (int e = threadIdx.x; e < kTz * kTy * kTx; e += kBlock) {
    const int tx = e % kTx, ty = (e / kTx) % kTy, tz = e / (kTx * kTy);
    const int gx = x0 + tx, gy = y0 + ty, gz = z0 + tz;
    if (gx >= nx || gy >= ny || gz >= nz) continue;
    const int hx = tx + 1, hy = ty + 1, hz = tz + 1;
    const int side = s_node[hz][hy][hx] & kInside;
    auto valid = [&](int dx, int dy, int dz) { return (s_cell[hz + dz][hy + dy][hx + dx] & kValid) != 0; };
    uint8_t mask = 0;
    // x: (b, c) = (y, z);  y: (z, x);  z: (x, y).  The four cells n - e_b - e_c, n - e_c, n, n - e_b.
    if ((s_node[hz][hy][hx + 1] & kInside) != side && valid(0, -1, -1) && valid(0, 0, -1) && valid(0, 0, 0) && valid(0, -1, 0))
      mask |= 1;
    if ((s_node[hz][hy + 1][hx] & kInside) != side && valid(-1, 0, -1) && valid(-1, 0, 0) && valid(0, 0, 0) && valid(0, 0, -1))
      mask |= 2;
    if ((s_node[hz + 1][hy][hx] & kInside) != side && valid(-1, -1, 0) && valid(0, -1, 0) && valid(0, 0, 0) && valid(-1, 0, 0))
      mask |= 4;
    const size_t at = ((size_t)gz * (size_t)ny + (size_t)gy) * (size_t)nx + (size_t)gx;
    a.node_mask[at] = mask;
    a.node_tris[at] = (uint8_t)(2 * __popc((unsigned)mask));
  }
}

// --------------------------------------------------------------- emit ----
// One thread per cell; an active one (a small share) reads its 8 corners and
// writes its vertex at its rank.
template <bool COLOR>
__global__ __launch_bounds__(kBlock) void k_mesh_vertices(gs_mesh_args a) {
  const int cx = a.vol.nx - 1, cy = a.vol.ny - 1, cz = a.vol.nz - 1;
  const long long cells = (long long)cx * cy * cz;
  const long long c = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (c >= cells || !a.cell_active[c]) return;
  const int rank = a.cell_rank[c] - 1;
  if (rank < 0 || rank >= a.num_vertices) return;  // (prefix sums that are not this volume's)
  const int row = (int)(c / cx), i = (int)(c - (long long)row * cx);
  const int k = row / cy, j = row - k * cy;
  const size_t nx = (size_t)a.vol.nx, plane = nx * (size_t)a.vol.ny, nodes = plane * (size_t)a.vol.nz;
  const size_t base = (size_t)k * plane + (size_t)j * nx + (size_t)i;
  float f[8], col[COLOR ? 8 : 1][3];  // corner index: 4 dz + 2 dy + dx
#pragma unroll
  for (int q = 0; q < 8; ++q) {
    const size_t at = base + (size_t)(q >> 2) * plane + (size_t)((q >> 1) & 1) * nx + (size_t)(q & 1);
    f[q] = a.vol.tsdf[at];
    if constexpr (COLOR) {
#pragma unroll
      for (int ch = 0; ch < 3; ++ch) col[q][ch] = a.vol.color[(size_t)ch * nodes + at];
    }
  }
  float sx = 0.f, sy = 0.f, sz = 0.f, sc[3] = {0.f, 0.f, 0.f};
  int crossings = 0;
#pragma unroll
  for (int axis = 0; axis < 3; ++axis) {
#pragma unroll
    for (int o = 0; o < 4; ++o) {
      // the other two offsets (lexicographic): x edges (dy, dz), y edges (dx, dz), z edges (dx, dy)
      const int o0 = o >> 1, o1 = o & 1;
      const int dx = axis == 0 ? 0 : o0, dy = axis == 0 ? o0 : (axis == 1 ? 0 : o1), dz = axis == 2 ? 0 : o1;
      const int qa = 4 * dz + 2 * dy + dx, qb = qa + (axis == 0 ? 1 : (axis == 1 ? 2 : 4));
      const float fa = f[qa], fb = f[qb];
      if ((fa < 0.f) == (fb < 0.f)) continue;
      const float r = fa / (fa - fb);
      sx += (float)dx + (axis == 0 ? r : 0.f);
      sy += (float)dy + (axis == 1 ? r : 0.f);
      sz += (float)dz + (axis == 2 ? r : 0.f);
      if constexpr (COLOR) {
#pragma unroll
        for (int ch = 0; ch < 3; ++ch) sc[ch] += col[qa][ch] + r * (col[qb][ch] - col[qa][ch]);
      }
      ++crossings;
    }
  }
  const float inv = (float)crossings;  // >= 3 for an active cell
  const float h = a.vol.voxel_size;
  float *out = a.vertices + 3 * (size_t)rank;
  out[0] = a.vol.origin[0] + h * ((float)i + sx / inv);
  out[1] = a.vol.origin[1] + h * ((float)j + sy / inv);
  out[2] = a.vol.origin[2] + h * ((float)k + sz / inv);
  if constexpr (COLOR) {
    float *oc = a.colors + 3 * (size_t)rank;
#pragma unroll
    for (int ch = 0; ch < 3; ++ch) oc[ch] = sc[ch] / inv;
  }
}

// One thread per node; one with a mask reads the ranks of the cells around its
// emitting edges and writes two triangles for each.
__global__ __launch_bounds__(kBlock) void k_mesh_faces(gs_mesh_args a) {
  const int nx = a.vol.nx, ny = a.vol.ny;
  const long long nodes = (long long)nx * ny * a.vol.nz;
  const long long n = (long long)blockIdx.x * kBlock + threadIdx.x;
  if (n >= nodes) return;
  const int mask = a.node_mask[n];
  if (!mask) return;
  const int row = (int)(n / nx), i = (int)(n - (long long)row * nx);
  const int k = row / ny, j = row - k * ny;
  const long long cx = nx - 1, cy = ny - 1;
  int face = a.node_faces[n] - 2 * __popc((unsigned)mask);
  const bool inside = a.vol.tsdf[n] < 0.f;
  // (a set bit says the four cells exist: classify checked them)
  auto rank = [&](int ci, int cj, int ck) { return a.cell_rank[((long long)ck * cy + cj) * cx + ci] - 1; };
  auto emit = [&](int c00, int c10, int c11, int c01) {
    if (face < 0 || face + 2 > a.num_faces) return;  // (prefix sums that are not this volume's)
    int *out = a.faces + 3 * (size_t)face;
    out[0] = c00; out[1] = inside ? c10 : c11; out[2] = inside ? c11 : c10;
    out[3] = c00; out[4] = inside ? c11 : c01; out[5] = inside ? c01 : c11;
    face += 2;
  };
  if (mask & 1) emit(rank(i, j - 1, k - 1), rank(i, j, k - 1), rank(i, j, k), rank(i, j - 1, k));
  if (mask & 2) emit(rank(i - 1, j, k - 1), rank(i - 1, j, k), rank(i, j, k), rank(i, j, k - 1));
  if (mask & 4) emit(rank(i - 1, j - 1, k), rank(i, j - 1, k), rank(i, j, k), rank(i - 1, j, k));
}

// ------------------------------------------------------------- checks ----
gs_status check_volume(const gs_tsdf_volume &v, const char *what) {
  if (v.nx < 1 || v.ny < 1 || v.nz < 1)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: every volume dimension must be at least 1", what);
  if ((long long)v.nx * v.ny >= (1ll << 31) || (long long)v.nx * v.ny * v.nz >= (1ll << 31))
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: the volume must have fewer than 2^31 nodes", what);
  if (!(isfinite(v.voxel_size) && v.voxel_size > 0.f))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: voxel_size must be finite and > 0", what);
  if (!(isfinite(v.origin[0]) && isfinite(v.origin[1]) && isfinite(v.origin[2])))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: the origin must be finite", what);
  if (!v.tsdf || !v.weight) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null tsdf or weight", what);
  return GS_OK;
}

inline long long cells_of(const gs_tsdf_volume &v) { return (long long)(v.nx - 1) * (v.ny - 1) * (v.nz - 1); }
inline long long nodes_of(const gs_tsdf_volume &v) { return (long long)v.nx * v.ny * v.nz; }

}  // namespace

extern "C" gs_status gs_tsdf_integrate(const gs_tsdf_integrate_args *a, gs_stream_t stream) {
  static const char *what = "gs_tsdf_integrate";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (!(isfinite(a->trunc) && a->trunc > 0.f))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: trunc must be finite and > 0", what);
  if (!(isfinite(a->near) && a->near > 0.f))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: near must be finite and > 0", what);
  if (isnan(a->alpha_min) || isnan(a->depth_max))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: alpha_min and depth_max must not be NaN", what);
  if (gs_status s = check_volume(a->vol, what)) return s;
  if (a->num_views < 1 || a->width < 1 || a->height < 1)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: needs at least one view of at least 1x1", what);
  if ((long long)a->width * a->height >= (1ll << 31))
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: a view must have fewer than 2^31 pixels", what);
  if (!a->cameras || !a->depth) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null cameras or depth", what);
  IntegrateOrder o;
  const int by = (int)div_up(a->vol.ny, kIy);
  o.bx = (int)div_up(a->vol.nx, kIx);
  o.sy = min(kSy, by);
  o.sz = min(kSz, a->vol.nz);
  o.ty = (int)div_up(by, o.sy);
  const long long blocks = (long long)o.bx * o.sy * o.sz * o.ty * (long long)div_up(a->vol.nz, o.sz);
  if (blocks >= (1ll << 31))
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: the volume takes 2^31 or more workgroups of 64 x 4 x 1 nodes", what);
  o.blocks = (unsigned)blocks;
  if (a->vol.color && a->image)
    k_tsdf_integrate<true><<<o.blocks, kBlock, 0, (hipStream_t)stream>>>(*a, o);
  else
    k_tsdf_integrate<false><<<o.blocks, kBlock, 0, (hipStream_t)stream>>>(*a, o);
  return gs_internal_check_launch(what);
}

extern "C" gs_status gs_mesh_classify(const gs_mesh_args *a, gs_stream_t stream) {
  static const char *what = "gs_mesh_classify";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (gs_status s = check_volume(a->vol, what)) return s;
  if (isnan(a->min_weight)) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: min_weight must not be NaN", what);
  if (!a->node_tris || !a->node_mask || (!a->cell_active && cells_of(a->vol) > 0))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null cell_active, node_tris or node_mask", what);
  const dim3 tiles(div_up(a->vol.nx, kTx), div_up(a->vol.ny, kTy), div_up(a->vol.nz, kTz));
  if (tiles.y > 65535u || tiles.z > 65535u)
    return gs_internal_fail(GS_ERR_UNSUPPORTED, "%s: at most 65535 tiles of 8 nodes in y and of 4 in z", what);
  k_mesh_classify<<<tiles, kBlock, 0, (hipStream_t)stream>>>(*a);
  return gs_internal_check_launch(what);
}

extern "C" gs_status gs_mesh_emit(const gs_mesh_args *a, gs_stream_t stream) {
  static const char *what = "gs_mesh_emit";
  if (!a) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null args", what);
  if (gs_status s = check_volume(a->vol, what)) return s;
  if (a->num_vertices < 0 || a->num_faces < 0)
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: negative num_vertices or num_faces", what);
  if (a->num_vertices > cells_of(a->vol) || a->num_faces > 6 * nodes_of(a->vol))
    return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: more vertices than cells, or more faces than 6 a node", what);
  if (a->colors && !a->vol.color) return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: colors without a colour volume", what);
  if (a->num_vertices > 0) {
    if (!a->cell_active || !a->cell_rank || !a->vertices)
      return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null cell_active, cell_rank or vertices", what);
    const unsigned blocks = div_up(cells_of(a->vol), kBlock);
    if (a->colors)
      k_mesh_vertices<true><<<blocks, kBlock, 0, (hipStream_t)stream>>>(*a);
    else
      k_mesh_vertices<false><<<blocks, kBlock, 0, (hipStream_t)stream>>>(*a);
    if (gs_status s = gs_internal_check_launch(what)) return s;
  }
  if (a->num_faces > 0) {
    if (!a->node_mask || !a->node_faces || !a->cell_rank || !a->faces)
      return gs_internal_fail(GS_ERR_INVALID_ARG, "%s: null node_mask, node_faces, cell_rank or faces", what);
    k_mesh_faces<<<div_up(nodes_of(a->vol), kBlock), kBlock, 0, (hipStream_t)stream>>>(*a);
    return gs_internal_check_launch(what);
  }
  return GS_OK;
}
