/*
 * gsplat_mi355x.h -- C ABI of the MI355X (gfx950) Gaussian-splatting rasterizer.
 *
 * Drop-in boundary for GaussianRenderer.render() of
 * Loveof1ife7/mini-3d-gaussian-splatting (src/core/renderer.py:31-367) and the
 * autograd backward the reference gets from torch.  Every stage of the
 * reference's render pipeline maps to one entry point below; each entry
 * point cites the reference function it replaces.
 *
 * Conventions
 *  - Plain C: raw device pointers, sizes, POD structs.  No torch types.
 *  - Stream ordered: every function enqueues work on `stream` (a hipStream_t
 *    passed as void*) and returns without synchronising.
 *  - Caller owns all memory.  The library never allocates; scratch comes from
 *    caller-provided workspaces whose sizes the *_workspace_bytes() queries
 *    return.
 *  - Errors: every entry point returns a gs_status; gs_last_error() returns a
 *    thread-local message for the last non-OK status on the calling thread.
 *    Nothing aborts or exits.
 *  - Re-entrant: no mutable globals; safe from several host threads on
 *    different streams.
 *  - fp32 throughout (the reference computes in fp32).
 */
#ifndef GSPLAT_MI355X_H
#define GSPLAT_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GS_ABI_VERSION 23
#define GS_DEFAULT_TILE 16    /* renderer.py:24 tile_size default */
#define GS_MAX_TILE 16384     /* tile_size in [1, GS_MAX_TILE]; the reference accepts any int, and a tile
                                 of at least max(W, H) renders the same as any larger one (one tile
                                 holds the image), so callers clamp to max(W, H): images up to
                                 16384 px on an edge render as one tile (ceil(L/8)^2 <= 4.2 M cells;
                                 the blend launches one 64-lane workgroup per cell of 8 tile slots,
                                 and a launch's work-items stay below 2^32) */
#define GS_QUAD 8             /* pixel cells of 8x8, laid out from each tile's origin: a tile of
                                 edge L holds gs_tile_quads(L) = ceil(L/8)^2 of them (edge cells
                                 clipped to the tile); one 64-lane wave renders one cell */
#define GS_MAX_TILES_AXIS 4096 /* ceil(W/L), ceil(H/L) <= 4096 (12-bit tile coordinates) */
#define GS_MAX_RECT_TILES 256 /* a Gaussian's tile rectangle spans <= 256 tiles in x: holds for
                                 any radius_max when ceil(W/L) <= 256, else needs
                                 ceil((2 floor(radius_max) + 1) / L) + 1 <= 256;
                                 gs_project_forward returns GS_ERR_UNSUPPORTED otherwise */
#define GS_RECORD_FLOATS 12   /* per-Gaussian splat record (3 x float4), see DESIGN.md */
#define GS_PAIR_GRAD_FLOATS 10 /* per (list entry, partial group) gradient partial (gs_partial_groups) */
#define GS_PARTIAL_STRIDE 10   /* floats between partials in pair_grads (dense: 40 B each) */
#define GS_NUM_COUNTERS 8     /* [0] visible M, [1] tile touches T, [2] / [3] min / max fp32 bits of the
                                 visible depths (0xFFFFFFFF / 0 when none; see gs_project_args),
                                 [4] the frame status (GS_FRAME_* bits below), [5] the list entries the
                                 later stages use: T, or 0 when the status is non-zero; [6..7] unused */
/* Frame status bits (gs_bin_count, counters[4]): what a device-resident frame
 * (gs_render_fwd_args.device_counts) could not do on the device.  A frame
 * with a non-zero status is drawn with empty tile lists (memory-safe); its
 * image, alpha and depth are those of a frame that draws nothing (the
 * background once, zeros: renderer.py:74-83, what the host path returns at
 * M == 0), and its caller renders it again on the host path. */
#define GS_FRAME_NEED_CAPACITY 1u /* T > the tile workspace's capacity */
#define GS_FRAME_WINDOW_MISS 2u   /* a visible depth left the depth-key window (or an MSD bucket overflowed) */
#define GS_FRAME_EMPTY 4u         /* M == 0: nothing to draw (renderer.py:74-83's background image) */

typedef enum gs_status {
  GS_OK = 0,
  GS_ERR_INVALID_ARG = 1,
  GS_ERR_LAUNCH = 2,
  GS_ERR_UNSUPPORTED = 3,
  /* gs_render_forward only -- not errors, what the caller does next: */
  GS_NEED_CAPACITY = 4,   /* T list entries exceed the tile workspace: grow it and call again with resume = 1 */
  GS_RETRY_FULL_KEYS = 5  /* a visible depth left the depth-key window: render again with key_bits = 32 */
} gs_status;

typedef void *gs_stream_t; /* hipStream_t */

/* Camera + settings as the reference renderer reads them.
 * fx,fy,cx,cy come from camera._width/_height/_FoVx/_FoVy exactly as
 * renderer.py:140-147 computes them (python double, rounded to fp32);
 * view is rows 0..2 of camera.world_view_transform() (renderer.py:150-152,
 * untransposed, column-vector convention). */
typedef struct gs_camera {
  int32_t image_width;   /* RenderSettings.image_width  (renderer.py:60) */
  int32_t image_height;  /* RenderSettings.image_height */
  float fx, fy, cx, cy;
  float view[12];        /* row-major 3x4 [R | t] */
  float radius_min;      /* GaussianRenderer(radius_min=0.01) */
  float radius_max;      /* GaussianRenderer(radius_max=50.0): finite, >= radius_min (see GS_MAX_RECT_TILES) */
  float bg[3];           /* RenderSettings.bg_color */
  int32_t tile_size;     /* GaussianRenderer(tile_size=16): 1..GS_MAX_TILE */
  float campos[3];       /* camera centre in world coordinates, -R^T t; read only when sh_degree > 0 */
} gs_camera;

/* Gaussian inputs (the duck-typed GaussianModel accessors).
 * Covariance: either cov3d ([n,9] row-major, = get_covariance) or the raw
 * parameters scaling ([n,3] log-sigma) + rotation ([n,4] q=[w,x,y,z], not
 * necessarily normalised), from which the kernel builds
 * R(normalize(q)) diag(exp(s)^2) R^T as gaussian_model.py:200-207 does. */
typedef struct gs_gaussians {
  int32_t n;
  const float *xyz;          /* [n, xyz_stride] get_xyz */
  int64_t xyz_stride;        /* floats between rows (3 if contiguous) */
  const float *cov3d;        /* [n,9] or NULL */
  const float *scaling;      /* [n,3] raw, used when cov3d == NULL */
  const float *rotation;     /* [n,4] raw, used when cov3d == NULL */
  const float *color_logits; /* [n, color_stride] get_features[:,0,:] (pre-sigmoid, renderer.py:88-92) */
  int64_t color_stride;
  const float *opacity;      /* [n, opacity_stride] get_opacity.squeeze(1) as given (renderer.py:94) */
  int64_t opacity_stride;
  int32_t opacity_is_logit;  /* 1: opacity holds the model's raw _opacity; the kernels apply
                                get_opacity's sigmoid (gaussian_model.py:119-120) and d_opacity
                                is the gradient w.r.t. the logit */
  /* View-dependent colour (off by default).  The reference
   * renders sigmoid(features[:,0,:]) only (renderer.py:88-92; its
   * MathUtils.spherical_harmonics_eval returns coeffs[:,0], math_utils.py:45-49).
   * sh_degree = 0 is exactly that.  sh_degree = d in 1..3 evaluates the
   * degree-d real SH of the view direction dir = normalize(xyz - campos):
   *   logit_c = color_logits[c] + sum_{k=1}^{(d+1)^2-1} Y_k(dir) sh_rest[k-1][c]
   * (Y_k: the 3DGS basis constants and signs; the DC coefficient stays the
   * raw logit, so degree 0 reduces to the reference), colour = sigmoid(logit). */
  int32_t sh_degree;
  const float *sh_rest;      /* [n, sh_rest_stride] rows holding [15,3] (get_features[:,1:,:]) */
  int64_t sh_rest_stride;
} gs_gaussians;

/* Screen-space low-pass filter (anti-aliasing; not in the reference).  With
 * V0 = J cov_cam J^T + 1e-6 I (renderer.py:182-183), the projection works on
 *   V = V0 + variance I
 * wherever it read cov2d: the conic Q = inv(V) (the full 2x2 inverse), lmax,
 * the radius and its clamp, the cull test, the tile rectangle, the depth key.
 * With compensate != 0 the opacity written to the splat record is
 *   opacity rho,  rho = sqrt(max(det V0 / det V, 2.5e-5))
 * (after get_opacity's sigmoid when opacity_is_logit; determinants in double
 * from the fp32 entries; the floor is Mip-Splatting's), so that a splat keeps
 * its energy; nothing else reads rho.  variance: px^2, >= 0 and finite
 * (0.3: 3DGS's dilation, 0.1: Mip-Splatting's); 0 is off whatever compensate
 * says -- all zero is the unfiltered projection, bit for bit.  The blend, the
 * feature replay, the gather and the density statistics read the record and
 * the outputs: they do not know of the filter. */
typedef struct gs_screen_filter {
  float variance;
  int32_t compensate;
} gs_screen_filter;

/* ---- Stage 1: _project_gaussians_3d_to_2d + _frustum_culling ----------
 * Replaces renderer.py:117-200 and :201-220.  One thread per Gaussian.
 * Writes the render() outputs means2d (viewspace_points), conics, radii and
 * visibility_filter, plus the splat record, tile rectangle and depth sort
 * key used by the later stages.  No atomics, no counters: the visible
 * count is produced by gs_bin_count.
 * filter (gs_screen_filter): cov2d = V0 + variance I for the conic, the
 * radius, the cull test, the rectangle and the key, and the record's opacity
 * times rho when compensating.  A negative or non-finite variance:
 * GS_ERR_INVALID_ARG before any HIP call. */
typedef struct gs_project_args {
  gs_camera cam;
  gs_gaussians g;
  float *means2d;       /* [n,2] */
  float *conics;        /* [n,4] = [n,2,2] */
  float *radii;         /* [n]   */
  uint8_t *vis;         /* [n]   torch.bool storage */
  float *records;       /* [n, GS_RECORD_FLOATS] */
  uint32_t *rects;      /* [n,2] packed tile rectangle */
  uint32_t *depth_keys; /* [n]   depth sort keys, see key_base */
  /* Depth keys for the sort of renderer.py:231-237.  Z > 0 for a visible
   * Gaussian, so the fp32 bits of Z order as the depths do: a visible g gets
   * depth_keys[g] = bits(Z) - key_base, a culled one 2^key_bits - 1 (last).
   * key_base = 0, key_bits = 32 is the plain float order.  A caller that
   * knows the visible depth range (counters[2..3] of the previous frame,
   * gs_bin_count) may window it to fewer bits and sort bits [0, key_bits):
   * one radix pass less per 8 bits.  The keys are exact only if every
   * visible bits(Z) - key_base < 2^key_bits - 1, which this frame's
   * counters[2..3] tell after gs_bin_count: otherwise sort again with 32. */
  uint32_t key_base;
  int32_t key_bits;     /* 1..32 */
  uint32_t *key_minmax; /* [2 * ceil(n / 256)] per-block min / max of the visible bits(Z), for
                           gs_bin_count's counters[2..3] */
  gs_screen_filter filter; /* all zero: none */
} gs_project_args;
gs_status gs_project_forward(const gs_project_args *a, gs_stream_t stream);

/* ---- Stage 2 / 4: device LSD radix sort (u32 key, u32 value) -----------
 * Replaces torch.argsort in _sort_gaussians_by_depth (renderer.py:231-237)
 * and the per-tile list build (:277-298).  Stable.  Sorts bits
 * [begin_bit, end_bit) of keys in ceil((end-begin)/8) passes, ping-ponging
 * between (keys, vals) and (keys_alt, vals_alt); *result_in_alt tells the
 * caller which pair holds the result (known on the host without a sync).
 * vals_are_iota != 0: the first pass reads values 0..n-1 instead of vals
 * (vals is still used as ping-pong storage). */
size_t gs_radix_sort_workspace_bytes(int32_t n);
gs_status gs_radix_sort_pairs(uint32_t *keys, uint32_t *vals, uint32_t *keys_alt,
                              uint32_t *vals_alt, int32_t n, int32_t begin_bit,
                              int32_t end_bit, int32_t vals_are_iota, void *workspace,
                              size_t workspace_bytes, int32_t *result_in_alt,
                              gs_stream_t stream);

/* Windowed depth keys (9 <= key_bits <= 32, gs_project_args.key_bits): the
 * same result as gs_radix_sort_pairs(keys, vals, keys_alt, vals_alt, n, 0,
 * key_bits, 1, ...) -- values = input positions, stable -- in one 8-bit MSD
 * pass plus one LDS-resident sort per top-digit bucket (one workgroup each).
 * The result is always in (keys_alt, vals_alt) (*result_in_alt = 1).
 * Preconditions: visible keys < 255 << (key_bits - 8); 2^key_bits - 1 is the
 * culled sentinel (its bucket stays in index order).  A bucket of more than
 * 16384 keys is left unsorted and 0xFFFFFFFF is stored to *overflow_word
 * (renderer: the depth-max word of gs_project_args.key_minmax, so the frame's
 * window check fails and it is sorted again with gs_radix_sort_pairs).
 * The buckets are sorted by the low key_bits - 8 bits in ceil((key_bits - 8)
 * / 8) LDS passes.  Workspace: gs_radix_sort_workspace_bytes(n).  key_bits
 * outside 9..32 returns GS_ERR_UNSUPPORTED. */
gs_status gs_depth_sort_msd(uint32_t *keys, uint32_t *vals, uint32_t *keys_alt, uint32_t *vals_alt,
                            int32_t n, int32_t key_bits, void *workspace, size_t workspace_bytes,
                            uint32_t *overflow_word, int32_t *result_in_alt, gs_stream_t stream);

/* ---- Stage 3: tile binning (renderer.py:263-298) ----------------------
 * gs_bin_count: per-Gaussian tile-touch counts and visibility in depth order,
 *   reduced to per-block partial sums and scanned; the callee zeroes
 *   counters, then counters[0] = M (visible), counters[1] = T (touches).
 *   It also numbers the gradient slots (one per touched tile) in
 *   Gaussian-index order, a Gaussian's slots consecutive: pair_offset is
 *   written here (chunk-local) and completed by gs_bin_emit.
 * gs_bin_emit : one (tile id, Gaussian id) entry per touched tile, emitted in
 *   depth order (so a stable sort by tile keeps depth order inside a tile),
 *   written coalesced; pair_offset[g] = g's first gradient slot, also stored
 *   in the Gaussian's record (word 10) for the backward's slot addressing. */
size_t gs_bin_workspace_bytes(int32_t n);
typedef struct gs_bin_args {
  int32_t n;
  int32_t tiles_x, tiles_y;
  const uint32_t *sorted_ids; /* [n] depth-sorted Gaussian ids (visible first) */
  const uint32_t *rects;      /* [n,2] from gs_project_forward (cleared by gs_bin_emit of a failed
                                 device-resident frame, see device_counts) */
  const uint8_t *vis;         /* [n]   from gs_project_forward */
  uint32_t *counters;         /* [GS_NUM_COUNTERS] */
  const uint32_t *key_minmax; /* gs_project_args.key_minmax (reduced into counters[2..3]) */
  void *workspace;             /* gs_bin_workspace_bytes(n); gs_bin_count leaves the per-block
                                  partials and the depth-ordered rectangles there for gs_bin_emit:
                                  pass the same workspace to both, untouched in between */
  size_t workspace_bytes;
  /* emit outputs (tile_keys / pair_gauss / records ignored by gs_bin_count) */
  uint32_t *tile_keys;   /* [T] */
  uint32_t *pair_gauss;  /* [T] */
  uint32_t *pair_offset; /* [n] indexed by Gaussian id: first gradient slot (both calls write it) */
  float *records;        /* [n, GS_RECORD_FLOATS]: word 10 <- pair_offset bits */
  int64_t capacity;      /* entries tile_keys / pair_gauss hold.  gs_bin_emit does nothing
                            when T = counters[1] > capacity, so it may be queued before T is
                            read back (then emit again into buffers of >= T entries) */
  uint32_t *host_counters; /* optional [8]: the device address of pinned host memory
                              (hipHostGetDevicePointer) that gs_bin_count also writes
                              counters[0..3] to, then -- after a system-scope fence --
                              host_seq to [4]: the caller polls [4] for the value it passed
                              and reads (M, T) with no copy and no event in the stream.
                              NULL: counters only */
  uint32_t host_seq;
  /* The frame status (counters[4], GS_FRAME_*), formed by gs_bin_count from
   * (M, T, the depth range) against capacity and the depth-key window the
   * keys were cut to (gs_project_args.key_base / key_bits): */
  uint32_t key_base;
  int32_t key_bits;        /* 0: no window check */
  uint32_t *step_flags;    /* optional device word: the status is ORed into it (sticky until the caller
                              clears it; gs_adam_args.skip_flag reads it) */
  int32_t device_counts;   /* a device-resident frame (gs_render_fwd_args.device_counts): when the
                              status is non-zero, gs_bin_emit emits nothing and clears every
                              rectangle (rects), so that the frame's backward gathers zero slots --
                              none past the capacity -- and the caller redoes the frame */
  uint32_t *frame_seq;     /* optional device word: incremented by every gs_bin_count; its new value is
                              written to host_counters[4] in place of host_seq (a captured graph
                              replays one frame per value).  host_counters also gets [5] the status,
                              [6] the step flags after this frame (the status without step_flags) and,
                              when this frame is the first to set them, [7] its sequence value */
} gs_bin_args;
gs_status gs_bin_count(const gs_bin_args *a, gs_stream_t stream);
gs_status gs_bin_emit(const gs_bin_args *a, gs_stream_t stream);

/* Per-tile [start,end) ranges of the tile-sorted entries.  Replaces the
 * tile_lists of renderer.py:266 (the sorted values are the Gaussian ids). */
typedef struct gs_range_args {
  int32_t num_pairs;           /* T */
  int32_t num_tiles;
  const uint32_t *sorted_keys; /* [T] tile ids, sorted */
  uint32_t *ranges;            /* [num_tiles,2] */
  uint8_t *slot_live;          /* optional (NULL: none): zeroed here, [T, cells] -- the backward's
                                  gs_blend_bwd_args.slot_live, cleared without a kernel of its own */
  int32_t cells;               /* gs_partial_groups(tile_size), with slot_live */
  const uint32_t *num_pairs_dev; /* optional device word (counters[5]): the entries are
                                  min(*num_pairs_dev, num_pairs), num_pairs only bounding them (a
                                  launch sized by capacity before T is known on the host) */
} gs_range_args;
gs_status gs_tile_ranges(const gs_range_args *a, gs_stream_t stream);

/* ---- Stage 5: _tile_rasterization blend, forward -------------------------
 * renderer.py:273-367: per pixel (integer coordinates) front-to-back alpha
 * compositing of its tile's list, termination once A >= 0.995, background
 * composite (bg counted twice, as the reference does), clamps, depth
 * normalisation.  One 64-lane workgroup per (tile, 8x8 cell), the cells of
 * a tile independent of each other, each walking the tile's list.  What the
 * backward needs beside the outputs themselves: pix_flags (one byte per
 * pixel: which clamps blocked), cell_neval (per cell, the evaluated prefix)
 * and the liveness bitmap. */
typedef struct gs_blend_fwd_args {
  gs_camera cam;
  int32_t tiles_x, tiles_y;
  const uint32_t *ranges;       /* [num_tiles,2] */
  const uint32_t *sorted_gauss; /* [T] */
  const float *records;         /* [n, GS_RECORD_FLOATS] */
  float *image;                 /* [3,H,W] */
  float *alpha;                 /* [H,W]   */
  float *depth;                 /* [H,W]   */
  uint8_t *pix_flags;           /* [H*W] the backward's per-pixel state beside the outputs: bit c
                                   (c = 0..2) set where channel c's composite left [0, 1] (its clamp
                                   blocks the gradient), bit 3 likewise for alpha */
  uint32_t *cell_neval;         /* [num_tiles * gs_tile_quads(tile_size)]: per (tile, 8x8 cell q),
                                   at tile * cells + q, the entries of the tile's list up to the last
                                   one any of the cell's pixels evaluated: the largest pix_neval
                                   among the cell's pixels inside the tile and the image (the
                                   list's length if one of them never reached A >= 0.995; 0 for a
                                   cell wholly outside) */
  uint64_t *live_bits;          /* [gs_tile_quads(tile_size), live_words]: see gs_blend_live_words;
                                   NULL: none written (a caller's memory budget for large tiles; the
                                   backward then replays every entry of a cell's evaluated prefix) */
  int64_t live_words;
  uint32_t *pair_counts;        /* [H*W] or NULL: each pixel's contributing pairs (c > 0), the
                                   work counter C of SURVEY 8(d); measurement only */
  int32_t num_pairs;            /* T, the entries of sorted_gauss: tile ranges are clamped to it */
  uint32_t *pix_neval;          /* [H*W] or NULL: each pixel's evaluated entries (the work counter
                                   E of SURVEY 8(d), and the oracle's decision-forced replay): 1 +
                                   the list index of the entry after which the pixel's A reached
                                   0.995, or the length of its tile's list if it never did (entries
                                   skipped on the way count); measurement only */
} gs_blend_fwd_args;
gs_status gs_blend_forward(const gs_blend_fwd_args *a, gs_stream_t stream);

/* Words per cell of the liveness bitmap the forward writes for the
 * backward: bit i of live_bits[q * live_words + ranges[2t] / 64 + t + i / 64]
 * is set iff list entry i of tile t reached (exp(-s/2) >= 1e-5) some
 * still-running pixel of the tile's 8x8 cell q = qx + qy * ceil(L/8)
 * (pixels [qx*8, qx*8+8) x [qy*8, qy*8+8) from the tile's origin) -- the
 * backward replays exactly those (entry, cell) pairs.  Bits past a cell's
 * last evaluated entry are left unwritten. */
size_t gs_blend_live_words(int32_t num_pairs, int32_t num_tiles);
/* Cells per tile: ceil(tile_size / 8)^2 (4 for the default 16); 0 if out of range. */
int32_t gs_tile_quads(int32_t tile_size);
/* Gradient partials a one-batch gs_blend_backward writes per list entry: one
 * per 8x8 cell, gs_tile_quads(tile_size) (4 for the default 16x16 tile); 0 if
 * out of range.  A caller whose [T, cells] partial buffer would not fit its
 * memory budget (large tiles: (L/8)^2 cells) replays the cells in batches
 * (gs_blend_bwd_args.cell_begin / cell_count), summing each batch with
 * gs_gather_partials(accumulate) before the next: bounded memory, the same
 * fixed summation order on every run (deterministic at every tile size). */
int32_t gs_partial_groups(int32_t tile_size);

/* ---- Backward of the blend -------------------------------------------
 * Re-walks each pixel's list front-to-back (bit-identical replay of the
 * forward's decisions) over the entries the forward's liveness bitmap marks
 * for its 8x8 cell, and writes one partial gradient per (entry, partial
 * group): pair_grads[G e + q] = {dmu_x, dmu_y, dQ00, dQ01(=dQ10), dQ11,
 * d_opacity, d_r, d_g, d_b, d_z} summed over group q's pixels, and sets
 * slot_live[G e + q] = 1; G = gs_partial_groups(tile_size), e = the entry's
 * gradient slot (pair_offset[g] + its tile's index in g's rectangle).  One
 * 64-lane workgroup per (tile, cell), and the group is the cell.  Groups
 * that did not replay the entry write nothing.  No atomics: deterministic.
 * A launch replays the cells [cell_begin, cell_begin + cell_count) of every
 * tile (cell_count 0 with cell_begin 0: all of them); G is then cell_count
 * and group q - cell_begin holds cell q's partial. */
typedef struct gs_blend_bwd_args {
  gs_camera cam;
  int32_t tiles_x, tiles_y;
  const uint32_t *ranges;
  const uint32_t *sorted_gauss;
  const float *records;         /* with pair offsets (gs_bin_emit) */
  const float *image;           /* the forward's outputs, unmodified */
  const float *alpha;
  const float *depth;
  const uint8_t *pix_flags;     /* gs_blend_fwd_args.pix_flags / cell_neval of the same forward */
  const uint32_t *cell_neval;
  const float *g_image;         /* [3,H,W] dL/dimage */
  const float *g_alpha;         /* [H,W] or NULL */
  const float *g_depth;         /* [H,W] or NULL */
  const uint64_t *live_bits;    /* the forward's liveness bitmap */
  int64_t live_words;
  float *pair_grads;            /* [T, G, GS_PARTIAL_STRIDE], G = the batch's cell_count */
  uint8_t *slot_live;           /* [T, G], zeroed by the caller (or gs_tile_ranges) */
  int32_t num_pairs;            /* T, the entries of sorted_gauss: tile ranges are clamped to it */
  int32_t cell_begin;           /* the batch's first cell (0) */
  int32_t cell_count;           /* the batch's cells (0: gs_tile_quads(tile_size), the whole tile) */
} gs_blend_bwd_args;
gs_status gs_blend_backward(const gs_blend_bwd_args *a, gs_stream_t stream);
/* gs_blend_backward with the absolute screen-space gradients (AbsGS; gsplat's
 * absgrad) beside the partials: everything above is written as there, bit for
 * bit (the same checks, cell batches and grid), and for every (entry, group)
 * whose slot_live flag it sets also
 *   abs_grads[2 (G e + q) + 0] = sum_p |dL/dmu_x(p)|
 *   abs_grads[2 (G e + q) + 1] = sum_p |dL/dmu_y(p)|
 * over group q's pixels p, where dL/dmu(p) is pixel p's own term of
 * pair_grads' dmu_x, dmu_y (their sum over p): the signed sum lets a large
 * Gaussian's per-pixel gradients cancel, this one does not.  Per pixel:
 * |dL/ds(p)| |(2 Q00 dx + (Q01+Q10) dy, (Q01+Q10) dx + 2 Q11 dy)|, (dx, dy)
 * the forward's own offsets.  abs_grads: device [T, G, 2] fp32, 8-byte
 * aligned; entries whose flag stays 0 are not written.  The colour pass only:
 * the feature and distortion backwards have no absolute form.  A NULL or
 * misaligned abs_grads: GS_ERR_INVALID_ARG before any HIP call. */
gs_status gs_blend_backward_abs(const gs_blend_bwd_args *a, float *abs_grads, gs_stream_t stream);
/* Diagnostic (SURVEY 8(d) lane efficiency; not on the render path): the same
 * replay as gs_blend_backward at the default tile (one batch), counting its
 * phase-A lanes.  hist: device [2][65] uint64, added to -- per replayed
 * (entry, cell), [0][r] counts replays entered by r running lanes (lanes of
 * the cell's pixels whose transmittance has not terminated), [1][c] replays
 * where c lanes' pairs contribute (weight > 0).  per_group: device [G][4]
 * uint32 overwritten, G = gs_blend_backward_groups(tiles_x, tiles_y, 4),
 * workgroup b = (tile, cell) per gs_blend_backward's grid: replays, replays
 * entered with >= 32 running lanes, sum of running lanes, sum of
 * contributing lanes (empty workgroups: zeros).  The gradient partials are
 * written as by gs_blend_backward. */
int64_t gs_blend_backward_groups(int32_t tiles_x, int32_t tiles_y, int32_t cell_count);
gs_status gs_blend_backward_lane_stats(const gs_blend_bwd_args *a, uint64_t *hist, uint32_t *per_group,
                                       gs_stream_t stream);

/* ---- The colour forward's saved state, as every replay reads it ------------
 * The passes below (feature channels, contribution statistics, depth
 * distortion) evaluate no transmittance chain of their own: they replay the
 * decisions of the gs_blend_forward that wrote ranges / sorted_gauss /
 * records / cell_neval / live_bits, bit for bit, as gs_blend_backward does --
 * one 64-lane workgroup per (tile, 8x8 cell), any tile_size; live_bits NULL:
 * every entry of a cell's evaluated prefix.  gs_replay_frame is that state;
 * it is the first member `f` of each pass's argument struct.  Every entry
 * point checks it the same way, before any HIP call: the camera
 * (GS_ERR_UNSUPPORTED), tiles_x / tiles_y against the image, a NULL ranges,
 * records or cell_neval, live_bits without live_words, a negative count
 * (GS_ERR_INVALID_ARG); a backward needs sorted_gauss and num_gaussians >= 1
 * always, a forward-type pass needs sorted_gauss only when num_pairs > 0.
 * (Source-level only: the nested struct occupies exactly the bytes the eleven
 * fields took when each struct spelled them out -- gs_camera is 108 bytes, the
 * frame ends at byte 176, 8-aligned -- so every later field keeps its offset
 * and GS_ABI_VERSION stays.) */
typedef struct gs_replay_frame {
  gs_camera cam;                /* the colour forward's (bg is not read) */
  int32_t tiles_x, tiles_y;
  const uint32_t *ranges;       /* as gs_blend_fwd_args, after that forward */
  const uint32_t *sorted_gauss;
  const float *records;         /* with pair offsets (gs_bin_emit) */
  const uint32_t *cell_neval;   /* gs_blend_fwd_args.cell_neval, as written */
  const uint64_t *live_bits;    /* gs_blend_fwd_args.live_bits, as written, or NULL */
  int64_t live_words;
  int32_t num_pairs;            /* T */
  int32_t num_gaussians;        /* n: the rows of a staged feature chunk */
} gs_replay_frame;

/* ---- Per-Gaussian feature channels through the blend ----------------------
 * features_out[k, p] = sum_i c_i F[g_i, k] over the entries i of pixel p's
 * tile list that the colour forward accepted, with the colour forward's own
 * contribution weights c_i (renderer.py:319-353: w = clamp(exp(-s/2), 0, 1),
 * skipped below 1e-5; alpha = clamp(o w, 0, 1); c = (1 - A) alpha; A += c,
 * break once A >= 0.995).  No background, clamp, sigmoid or normalisation: a
 * pixel no entry reaches gets 0.  The kernels replay the colour forward over
 * its saved state (gs_replay_frame).
 * Channels go in chunks of GS_FEATURE_CHUNK = 4, the payload width of the
 * colour pass (r, g, b, z), so a chunk's backward fits the 40-byte partial
 * and everything behind it.  `features` is the [n, C] input staged
 * chunk-major, [ceil(C / 4), n, 4] with the last chunk zero-padded: one
 * aligned 16-byte load per (entry, chunk).
 * GS_MAX_FEATURE_CHANNELS bounds C: 64 chunks, the forward's grid y axis, and
 * as many backward launches per cell batch -- wide enough for distilled
 * feature fields (CLIP / DINO embeddings are rendered at 16..256 channels),
 * small enough that a mistaken shape ([N, H W]) is refused, not launched. */
#define GS_FEATURE_CHUNK 4
#define GS_MAX_FEATURE_CHANNELS 256
typedef struct gs_feature_fwd_args {
  gs_replay_frame f;            /* the colour forward's saved state */
  int32_t channels;             /* C in 1..GS_MAX_FEATURE_CHANNELS */
  const float *features;        /* [ceil(C/4), n, 4] staged, 16-byte aligned */
  float *out;                   /* [C, H, W]: every pixel written */
} gs_feature_fwd_args;
/* Every chunk in one launch (chunks on the grid's y axis). */
gs_status gs_blend_features_forward(const gs_feature_fwd_args *a, gs_stream_t stream);

/* Backward of one chunk over one cell batch, for a cotangent g_out [C, H, W].
 * With X_i = sum_k g_out[k,p] F[g_i,k], K = sum_k g_out[k,p] out[k,p] and
 * P_i = sum_{j<=i} c_j X_j (k over the chunk's channels; the chunks add):
 *   dL/dF[g, k]  = sum_{p, i: g_i = g} c_i g_out[k, p]
 *   dL/dalpha_i  = T_i (X_i + (P_i - K) / T_{i+1})   (the terminating entry: T_i X_i)
 * chained into (dmu_x, dmu_y, dQ00, dQ01, dQ11, d_opacity) with the clamp
 * masks of gs_blend_backward -- its formula with bg = 0, no alpha cotangent,
 * no pixel clamp and a plain fourth channel where it has depth.  Writes one
 * partial per replayed (entry, cell) in gs_blend_backward's layout,
 * pair_grads[G e + q] = {dmu_x, dmu_y, dQ00, dQ01, dQ11, d_opacity, dF0, dF1,
 * dF2, dF3}, and sets slot_live[G e + q] = 1 (G = cell_count, q the cell's
 * index in the batch, e the entry's gradient slot).  No atomics. */
typedef struct gs_feature_bwd_args {
  gs_replay_frame f;            /* the colour forward's saved state */
  int32_t channels;             /* C */
  int32_t chunk;                /* 0 .. ceil(C/4) - 1: channels [4 chunk, 4 chunk + 4) */
  const float *features;        /* the forward's staged input */
  const float *out;             /* [C, H, W] the forward's output, unmodified */
  const float *g_out;           /* [C, H, W] dL/dout */
  float *pair_grads;            /* [T, G, GS_PARTIAL_STRIDE] */
  uint8_t *slot_live;           /* [T, G], zeroed by the caller */
  int32_t cell_begin;           /* the batch's first cell */
  int32_t cell_count;           /* the batch's cells (0 with cell_begin 0: the whole tile) */
} gs_feature_bwd_args;
gs_status gs_blend_features_backward(const gs_feature_bwd_args *a, gs_stream_t stream);

/* The gather of a feature chunk's partials: per Gaussian g, its slots' live
 * partials summed in gs_gather_partials' order (the same lanes per Gaussian,
 * slot and group order and lane tree).  Values 0..5 go to grad_sums[g, 0..5]:
 * stored, with grad_sums[g, 6..9] zeroed, when accumulate = 0; added, 6..9
 * left alone, when accumulate = 1 (the colour pass's sums, or an earlier
 * chunk's or batch's, are there).  Values 6..9 go to d_features[g,
 * channel_begin .. channel_begin + channel_count): stored when
 * feature_accumulate = 0 (a chunk's first cell batch), added when 1. */
typedef struct gs_feature_gather_args {
  int32_t n;
  const uint8_t *vis;           /* as gs_project_bwd_args */
  const uint32_t *rects;
  const uint32_t *pair_offset;
  const float *pair_grads;      /* [T, G, GS_PARTIAL_STRIDE] */
  const uint8_t *slot_live;     /* [T, G] */
  int32_t partial_groups;       /* G */
  int32_t accumulate;
  float *grad_sums;             /* [n, GS_PAIR_GRAD_FLOATS] */
  float *d_features;            /* [n, d_features_stride] */
  int64_t d_features_stride;    /* floats between rows */
  int32_t channel_begin;
  int32_t channel_count;        /* 1..GS_FEATURE_CHUNK */
  int32_t feature_accumulate;
} gs_feature_gather_args;
gs_status gs_gather_feature_partials(const gs_feature_gather_args *a, gs_stream_t stream);

/* ---- Per-Gaussian blend contribution statistics ---------------------------
 * How much each Gaussian contributes to a frame: a third replay of the
 * colour forward (gs_replay_frame), one 64-lane workgroup per (tile, 8x8
 * cell) of the cell batch [cell_begin, cell_begin + cell_count).
 * With c the forward's own contribution weight of an entry at a pixel
 * (c = (1 - A) alpha; +0 for a lane outside the tile or image, a skipped
 * pair or a terminated pixel), every replayed (entry, cell) writes
 *   partials[(slot G + q) GS_CONTRIB_STRIDE + 0] = sum over the cell's pixels of c (a fixed order)
 *                                            + 1] = max over the cell's pixels of c
 *                                            + 2] = pixels with c > 0 (a float, exact, <= 64)
 *                                            + 3] = 0 (reserved)
 *   slot_live[slot G + q] = 1
 * (one aligned 16-byte store; slot, G = cell_count and q as in
 * gs_blend_features_backward; cells that do not replay an entry write
 * nothing; no atomics).
 * dominant_id / dominant_weight (both or neither), [H*W]: per pixel of the
 * image the Gaussian of the entry with the largest c there (the first in
 * list order among equals) and that c; -1 / 0 where no entry has c > 0.
 * Every pixel of the batch's cells is written, those of empty tiles too.
 * n == 0 or num_pairs == 0: GS_OK, no partial is written, the maps are
 * filled with -1 / 0. */
#define GS_CONTRIB_STRIDE 4
typedef struct gs_contrib_args {
  gs_replay_frame f;            /* the colour forward's saved state */
  float *partials;              /* [T, G, GS_CONTRIB_STRIDE], 16-byte aligned */
  uint8_t *slot_live;           /* [T, G], zeroed by the caller */
  int32_t cell_begin;           /* the batch's first cell */
  int32_t cell_count;           /* the batch's cells (0 with cell_begin 0: the whole tile) */
  int32_t *dominant_id;         /* [H*W] or NULL */
  float *dominant_weight;       /* [H*W] or NULL (with dominant_id) */
} gs_contrib_args;
gs_status gs_blend_contributions(const gs_contrib_args *a, gs_stream_t stream);

/* One view's (or cell batch's) partials added to the running statistics:
 * per Gaussian g < n with vis[g] != 0, over its slots [pair_offset[g], +
 * touches) and the partial_groups groups slot_live flags, s = the sums added
 * in gs_gather_partials' slot, group and lane-tree order, m = the max,
 * k = the counts added; then
 *   weight_sum[g] += s, weight_max[g] = fmaxf(weight_max[g], m),
 *   pixels[g] += k, views[g] += first_batch ? 1 : 0.
 * A row with vis[g] == 0 is neither read nor written.  first_batch: 1 for a
 * view's first cell batch, 0 for its later ones. */
typedef struct gs_contrib_gather_args {
  int32_t n;
  const uint8_t *vis;           /* as gs_project_bwd_args */
  const uint32_t *rects;
  const uint32_t *pair_offset;
  const float *partials;        /* [T, G, GS_CONTRIB_STRIDE] */
  const uint8_t *slot_live;     /* [T, G] */
  int32_t partial_groups;       /* G */
  int32_t first_batch;
  float *weight_sum;            /* [n] */
  float *weight_max;            /* [n] */
  int64_t *pixels;              /* [n] */
  int32_t *views;               /* [n] */
} gs_contrib_gather_args;
gs_status gs_contrib_accumulate(const gs_contrib_gather_args *a, gs_stream_t stream);

/* ---- Depth distortion and median depth through the blend -------------------
 * How spread out along the ray a pixel's contributors are, and the depth of
 * the one surface at which its opacity crosses one half: a fourth replay of
 * the colour forward (gs_replay_frame), one 64-lane workgroup per (tile, 8x8
 * cell), lane = pixel.  With c_i the forward's own contribution weight of
 * entry i of the pixel's tile list (c = (1 - A) alpha, A = A + c; +0 for a
 * skipped pair, a terminated pixel, or a lane outside the tile or image),
 * z_i the camera-space depth in the entry's record (float 9) and m_i its
 * mapped depth,
 *   A_i = sum_{j<=i} c_j,   S_i = sum_{j<=i} c_j m_j   (A_0 = S_0 = 0)
 *   distortion(p) = 2 sum_i c_i (m_i A_{i-1} - S_{i-1})
 * The lists are sorted by the bits of z and both depth maps are monotone, so
 * this is the Mip-NeRF 360 / 2DGS distortion sum_i sum_j c_i c_j |m_i - m_j|;
 * a pixel with fewer than two contributors has 0.  The sum does not change
 * under a shift common to all m, and the kernels use one: every m is formed
 * directly as a difference to the pixel's first contributor f (the first
 * entry with c > 0, a decision of the replay, the same in both directions),
 *   linear  (near = far = 0):    m_i = z_i - z_f
 *   inverse (0 < near < far):    m_i = kappa (z_i - z_f) / (z_i z_f),  kappa = far near / (far - near)
 * the latter 2DGS's NDC depth far (z - near) / ((far - near) z) minus its
 * value at z_f.  Formed from unshifted fp32 values, m_i A - S loses a scene at
 * depth 2000 with a spread of 0.5 to cancellation, and the inverse map puts
 * everything into the last ulps below 1; as differences every term is
 * bounded by the pixel's own depth spread.
 * Median: the first entry with c_i > 0 after whose addition the fp32 running
 * A_i >= 0.5; if A never reaches 0.5, the last entry with c_i > 0; if there
 * is none, median_id = -1 and median_depth = 0.  median_depth is that
 * record's z, unmapped, bit for bit.
 * moments [2, H, W] = (A_n, S_n), the backward's state (A_n is the colour
 * forward's alpha, bit for bit; S_n is relative to z_f).  Every pixel of every
 * map is written.  n == 0 or num_pairs == 0: GS_OK, the maps are filled with
 * 0 / -1.  A NULL required pointer, or near / far neither both zero nor
 * finite with 0 < near < far: GS_ERR_INVALID_ARG before any HIP call. */
typedef struct gs_distortion_fwd_args {
  gs_replay_frame f;            /* the colour forward's saved state */
  float near, far;              /* both 0: linear depth; else the inverse map's planes */
  float *distortion;            /* [H, W] */
  float *moments;               /* [2, H, W]: A_n, S_n */
  float *median_depth;          /* [H, W] */
  int32_t *median_id;           /* [H, W] */
} gs_distortion_fwd_args;
gs_status gs_blend_distortion_forward(const gs_distortion_fwd_args *a, gs_stream_t stream);

/* Backward over one cell batch, for a cotangent g [H, W] on distortion.  With
 * A_n, S_n from moments and D = distortion(p):
 *   X_i = 2 g [m_i (A_{i-1} + A_i - A_n) + S_n - S_i - S_{i-1}]   (= g dD/dc_i)
 *   K   = 2 g D                                  (Euler: sum_i c_i X_i)
 *   dL/dalpha_i = T_i (X_i + (P_i - K) / T_{i+1}),  P_i = sum_{j<=i} c_j X_j
 *                                                (the terminating entry: T_i X_i)
 *   dL/dm_i = 2 g c_i (A_{i-1} + A_i - A_n)
 *   dL/dz_i = dL/dm_i * (1 | kappa / z_i^2)      (linear | inverse)
 * dL/dalpha_i is gs_blend_features_backward's formula with a per-pixel,
 * per-entry X_i in place of its dot product, chained with the same clamp
 * masks into (dmu_x, dmu_y, dQ00, dQ01, dQ11, d_opacity).  Nothing flows
 * through z_f: sum_i dL/dm_i = 0.  Writes one partial per replayed (entry,
 * cell) in gs_blend_backward's layout, pair_grads[G e + q] = {dmu_x, dmu_y,
 * dQ00, dQ01, dQ11, d_opacity, 0, 0, 0, d_z}, and sets slot_live[G e + q] = 1
 * (G = cell_count, q the cell's index in the batch, e the entry's gradient
 * slot).  No atomics.  gs_gather_partials(accumulate = 1) adds them to the
 * colour pass's sums (the three +0 leave its colour sums' bits alone), and
 * the projection backward, its pose form included, chains d_z. */
typedef struct gs_distortion_bwd_args {
  gs_replay_frame f;            /* the colour forward's saved state */
  float near, far;              /* the forward's */
  const float *distortion;      /* [H, W] the forward's output, unmodified */
  const float *moments;         /* [2, H, W] the forward's */
  const float *g_distortion;    /* [H, W] dL/ddistortion */
  float *pair_grads;            /* [T, G, GS_PARTIAL_STRIDE] */
  uint8_t *slot_live;           /* [T, G], zeroed by the caller */
  int32_t cell_begin;           /* the batch's first cell */
  int32_t cell_count;           /* the batch's cells (0 with cell_begin 0: the whole tile) */
} gs_distortion_bwd_args;
gs_status gs_blend_distortion_backward(const gs_distortion_bwd_args *a, gs_stream_t stream);

/* ---- Backward of the projection ----------------------------------------
 * Sums each Gaussian's slot partials (slots [pair_offset[g], pair_offset[g]
 * + touches), the groups slot_live flags), adds cotangents on the viewspace_points /
 * conics outputs, and chains through sigmoid(colour), inv(cov2d),
 * J cov_cam J^T, Rv Sigma Rv^T, the perspective Jacobian J(X,Y,Z) and
 * Xc = Rv Xw + Tv (autograd of renderer.py:117-200), and, on the raw path,
 * through Sigma(exp(s), normalize(q)) (gaussian_model.py:200-207), and with
 * sh_degree > 0 through the SH colour into sh_rest and (via the view
 * direction) into xyz.
 * filter: the forward's gs_screen_filter.  inv(cov2d) is inv(V0 + variance I)
 * (the raw path's double conic is rebuilt from it).  When compensating, with
 * acc[5] the blend's gradient at the record opacity:
 *   d_opacity = acc[5] rho (then the sigmoid chain),  d_rho = acc[5] opacity,
 * and, where the floor does not bind (r = det V0 / det V > 2.5e-5),
 *   d_V0 += d_rho / (2 rho) (adj(V0)^T / det V - r adj(V)^T / det V)
 * entry by entry (V[0][1] and V[1][0] are separate) before the chain into J
 * and cov_cam; where it binds rho is a constant.  A Gaussian whose only
 * cotangent is on opacity then has geometry gradients.  A negative or
 * non-finite variance: GS_ERR_INVALID_ARG before any HIP call. */
typedef struct gs_project_bwd_args {
  gs_camera cam;
  gs_gaussians g;
  const float *means2d, *conics; /* the forward's (required; the raw path forms its own conic, in double) */
  const uint8_t *vis;
  const uint32_t *rects;
  const uint32_t *pair_offset;
  const uint32_t *order;       /* [n] permutation to walk the Gaussians in (the gather and the
                                  projection backward), or NULL: index order (slots are numbered in
                                  index order, so NULL reads them coalesced) */
  const float *pair_grads;     /* [T,G,GS_PARTIAL_STRIDE] (G = partial_groups), summed into grad_sums
                                  first; NULL: no blend gradient (T == 0), or -- with grad_sums --
                                  the sums are already there (gs_gather_partials, cell batches) */
  const float *g_means2d;      /* [n,2] or NULL */
  const float *g_conics;       /* [n,4] or NULL */
  float *d_xyz;                /* [n,3] */
  float *d_cov3d;              /* [n,9]  (cov3d path) */
  float *d_scaling;            /* [n,3]  (raw path)   */
  float *d_rotation;           /* [n,4]  (raw path)   */
  float *d_color_logits;       /* [n,3] */
  float *d_opacity;            /* [n]   */
  float *d_sh_rest;            /* [n,15,3] contiguous, written when g.sh_degree > 0 (zeros past the degree) */
  const uint8_t *slot_live;    /* [T,G] from gs_blend_backward; required with pair_grads */
  float *grad_sums;            /* [n, GS_PAIR_GRAD_FLOATS]: g's partials summed (written first when
                                  pair_grads is given, else read as is); NULL: no blend gradient */
  int32_t partial_groups;      /* G of pair_grads / slot_live: the blend backward's cell_count */
  gs_screen_filter filter;     /* the forward's; all zero: none */
} gs_project_bwd_args;
gs_status gs_project_backward(const gs_project_bwd_args *a, gs_stream_t stream);
/* The gather alone: grad_sums[g] = (accumulate ? grad_sums[g] : 0) + the sum
 * of g's partials in pair_grads / slot_live (partial_groups per slot), for a
 * blend backward run in cell batches: batch b's sums are added after batch
 * b - 1's, a fixed order.  Reads vis, rects, pair_offset, g.n. */
gs_status gs_gather_partials(const gs_project_bwd_args *a, int32_t accumulate, gs_stream_t stream);
/* The same gather over gs_blend_backward_abs' absolute partials: for every
 * g < n, abs_sums[2g + k] = (accumulate ? abs_sums[2g + k] : 0) + the sum of
 * abs_grads[2 (G e + q) + k] over g's slots e and the groups q slot_live
 * flags, in gs_gather_partials' slot, group and lane order (fixed: no
 * atomics, bitwise reproducible; cell batches are added in batch order).  A
 * Gaussian that is invisible or has no live partial gets zeros when storing
 * and keeps its sums when accumulating.  Run it after each batch's
 * gs_blend_backward_abs, before slot_live is cleared for the next.  n == 0:
 * GS_OK, nothing launched. */
typedef struct gs_abs_gather_args {
  int32_t n;
  const uint8_t *vis;          /* [n] */
  const uint32_t *rects;       /* [n] packed tile rectangles */
  const uint32_t *pair_offset; /* [n] first slot */
  const float *abs_grads;      /* [T, G, 2] from gs_blend_backward_abs */
  const uint8_t *slot_live;    /* [T, G] */
  int32_t partial_groups;      /* G: the blend backward's cell_count */
  int32_t accumulate;          /* 0: store, 1: add to abs_sums */
  float *abs_sums;             /* [n, 2] */
} gs_abs_gather_args;
gs_status gs_gather_abs_partials(const gs_abs_gather_args *a, gs_stream_t stream);

/* ---- Backward of the projection, with the camera pose's gradient --------
 * gs_project_backward (every d_* of bwd is written as there, bit for bit)
 * plus dL/d(view) for cam.view = rows [R | t] of the world-to-camera matrix,
 * which the reference's autograd reaches through Xc = Rv Xw + Tv and
 * cov_cam = Rv Sigma Rv^T (renderer.py:150-168):
 *   d_t = sum_g dXc,  d_R = sum_g dXc Xw^T + dC (R Sigma^T) + dC^T (R Sigma)
 * and, with sh_degree > 0, through the view direction's origin
 * cam.campos = -R^T t:  d_R[i][j] -= t[i] d_campos[j],
 * d_t[i] -= sum_j R[i][j] d_campos[j].  R need not be orthonormal.
 * The sum over Gaussians is deterministic (no atomics): each workgroup of 256
 * Gaussians reduces in a fixed order into one row of pose_partials, and one
 * workgroup sums the rows in index order and a fixed tree, in double. */
typedef struct gs_project_pose_args {
  gs_project_bwd_args bwd;     /* as gs_project_backward; order must be NULL */
  double *pose_partials;       /* [pose_partial_rows, 16] workspace (contents undefined after the call) */
  int64_t pose_partial_rows;   /* >= ceil(bwd.g.n / 256) */
  float *d_view;               /* [12] out: rows [d_R | d_t], row-major 3x4 (zeros when bwd.g.n <= 0) */
} gs_project_pose_args;
gs_status gs_project_backward_pose(const gs_project_pose_args *a, gs_stream_t stream);

/* ---- Adam step over several parameter tensors, one launch -----------------
 * SURVEY 8(f) row 1 (fused Adam), the optimizer the reference builds in
 * src/core/optimizer.py:100-113 (torch.optim.Adam, 5 parameter groups).
 * torch.optim.Adam semantics (amsgrad off, weight_decay 0):
 *   m = b1 m + (1-b1) g ; v = b2 v + (1-b2) g^2
 *   p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps)
 * Tensors with grad == NULL are skipped (torch skips params without grad).
 * param_out: NULL updates p in place (torch's behaviour); otherwise p is
 * only read and the updated parameter is written to param_out (same
 * numel, no overlap with p) -- the same reads and writes as the in-place
 * step, e.g. for a benchmark that renders one fixed scene every step. */
#define GS_ADAM_MAX_TENSORS 8
typedef struct gs_adam_tensor {
  float *param, *exp_avg, *exp_avg_sq;
  const float *grad;     /* NULL: skip */
  int64_t numel;
  float lr;
  float bias_correction1; /* 1 - beta1^step */
  float bias_correction2_sqrt; /* sqrt(1 - beta2^step) */
  float *param_out;       /* NULL: in place */
} gs_adam_tensor;
typedef struct gs_adam_args {
  int32_t num_tensors;
  float beta1, beta2, eps;
  /* The gradient's weights 1 - beta1 and 1 - beta2, formed in double by the
   * caller and rounded once: 1.f - (float)0.999 is 1.3e-5 below 0.001, which
   * the second moment would carry while the bias corrections (formed in
   * double) assume 0.001.  0: 1.f - beta in fp32. */
  float one_minus_beta1, one_minus_beta2;
  gs_adam_tensor t[GS_ADAM_MAX_TENSORS];
  /* Replayed steps (a captured graph whose kernel arguments are fixed):
   * skip_flag: optional device word -- non-zero: the launch updates nothing
   *   (gs_bin_args.step_flags: the frame of this step failed on the device
   *   and the caller redoes the step on the host path);
   * hyper / hyper_row: optional -- tensor i's lr, bias_correction1 and
   *   bias_correction2_sqrt are read from hyper[(r * GS_ADAM_MAX_TENSORS + i)
   *   * 3 + 0..2], r = *hyper_row (a device word, e.g. gs_bin_args.frame_seq),
   *   instead of t[i]; the caller fills the rows the replays will reach. */
  const uint32_t *skip_flag;
  const float *hyper;
  const uint32_t *hyper_row;
} gs_adam_args;
gs_status gs_adam_step(const gs_adam_args *a, gs_stream_t stream);

/* Visibility-gated Adam (gsplat's visible_adam / SelectiveAdam, the sparse
 * Adam of Taming 3DGS): the update of gs_adam_step -- the same fp32
 * operations, lr, bias corrections and one_minus_beta* rounding -- on the
 * rows whose row_mask byte is non-zero only.  Every tensor with a grad is
 * [rows, cols[i]] row-major.  A row with row_mask[r] == 0 keeps the bits of
 * param, exp_avg and exp_avg_sq, and its gradient is never used (NaN / Inf
 * included; it is not even loaded where no element of its float4 is visible).
 * A workgroup owns GS_ADAM_ROW_BLOCK consecutive rows of one tensor: it reads
 * their mask bytes first and returns before any load of p, g, m or v when
 * none is set.  No atomics: bitwise reproducible, and bit-identical to
 * gs_adam_step on the visible rows.
 * param_out, skip_flag, hyper and hyper_row are not supported here
 * (GS_ERR_UNSUPPORTED when non-NULL), nor is cols[i] above
 * GS_ADAM_ROWS_MAX_COLS (the row of an element is found with a 32-bit
 * multiply-high, exact up to there).  GS_ERR_INVALID_ARG, before any HIP
 * call: NULL row_mask, rows < 0, cols[i] < 1, numel != rows * cols[i], a NULL
 * buffer behind a non-NULL grad.  rows == 0 or no tensor with a grad: GS_OK,
 * nothing launched. */
#define GS_ADAM_ROW_BLOCK 256          /* rows one workgroup owns; a multiple of 4 */
#define GS_ADAM_ROWS_MAX_COLS 2047
typedef struct gs_adam_rows_args {
  gs_adam_args adam;                   /* as gs_adam_step: betas, eps, one_minus_beta*, t[0..num_tensors) */
  int64_t rows;                        /* dim 0 shared by every tensor with a grad */
  int32_t cols[GS_ADAM_MAX_TENSORS];   /* t[i].numel == rows * cols[i], cols[i] >= 1 */
  const uint8_t *row_mask;             /* [rows]; non-zero: update the row */
} gs_adam_rows_args;
gs_status gs_adam_step_rows(const gs_adam_rows_args *a, gs_stream_t stream);

/* Optimizer in the backward (opt-in; one rank, no gradient hooks): the
 * projection backward of the training configuration (raw scaling / rotation,
 * opacity logit, DC colour, blend sums in grad_sums or pair_grads, no
 * viewspace / conic cotangents) applies the Adam update of gs_adam_step --
 * the same fp32 operations -- to each parameter where its gradient is formed,
 * instead of writing d_* (not read; no gradient reaches HBM).  adam->t[0..4]
 * are xyz, colour logits, opacity logit, scaling, rotation: param = the arrays
 * of a->g (dense rows), their moments, param_out (NULL: in place); grad is
 * ignored.  skip_flag / hyper / hyper_row as in gs_adam_args.  Saves the
 * gradients' write and read and the parameters' second read (~168 B per
 * Gaussian) and a launch.  GS_ERR_UNSUPPORTED outside that configuration. */
gs_status gs_project_backward_adam(const gs_project_bwd_args *a, const gs_adam_args *adam, gs_stream_t stream);

/* ---- Photometric loss ---------------------------------
 * total = (1 - lambda) * L1 + lambda * D-SSIM, the objective of GaussianLoss
 * (src/core/loss.py:41-63): L1 = mean |pred - target| (:56); D-SSIM =
 * 1 - mean(clamp(SSIM map, 0, 1)) over the statistics SSIMLoss builds
 * (:17-39): a K-tap Gaussian window with sigma = K/6, separable, zero
 * padding, C1 = 0.01^2, C2 = 0.03^2.  The reference SSIMLoss.forward ends
 * without a return; its caller consumes the value as `dssim` (:57-58), which
 * is the D-SSIM form implemented here.  Deterministic (fixed-order
 * reductions, no atomics). */
#define GS_LOSS_MAX_WINDOW 11
typedef struct gs_loss_args {
  int32_t channels, height, width; /* pred/target/d_pred: [C,H,W] fp32 contiguous */
  const float *pred, *target;
  float lambda_dssim;                /* loss.py:42 default 0.2 */
  int32_t window;                    /* odd, 1..GS_LOSS_MAX_WINDOW (loss.py:10 default 11) */
  float c1, c2;                      /* loss.py:14-15 */
  void *workspace;                   /* gs_loss_workspace_bytes */
  size_t workspace_bytes;
  float *maps;                       /* [3,C,H,W] written by the forward for the backward, or NULL */
  float *out;                        /* [3] total, l1, dssim (device) */
  const float *g_total;              /* backward: dL/dtotal (device scalar), NULL = 1 */
  float *d_pred;                     /* backward: [C,H,W] */
} gs_loss_args;
size_t gs_loss_workspace_bytes(int32_t channels, int32_t height, int32_t width);
gs_status gs_loss_forward(const gs_loss_args *a, gs_stream_t stream);
gs_status gs_loss_backward(const gs_loss_args *a, gs_stream_t stream);

/* ---- Densification ------------------------------------
 * One pass of split / clone / prune over the model's raw parameters
 * (gaussian_model.py:130-175 density_and_split / density_and_clone,
 * optimizer.py:64-66 opacity prune), with the Adam moments remapped: kept
 * Gaussians carry theirs, new ones start at zero.  Per Gaussian i, on the
 * pre-densify state: g = |dL/dxyz_i|, s = mean(exp(scaling_i));
 *   split = g > grad_threshold and s > split_size * scene_extent (:137):
 *     i is replaced by two children xyz -/+ R(q)[:,0] * 0.5 s, scaling
 *     log(0.75 exp(scaling)), rotation normalize(q), opacity
 *     clamp(logit(sigmoid(op)), -6, 6), features copied (:139-154);
 *   clone = g > grad_threshold and s < clone_size * scene_extent (:166):
 *     i stays and a copy is added at xyz + N(0,1)^3 * 0.5 s (:169-178);
 *   prune: every output whose sigmoid(opacity) <= min_opacity is dropped.
 * Output order: kept originals, split "-" children, split "+" children,
 * clones; each in the original index order.  (The reference cannot run
 * these: _append_points reads a missing `_scaling_log` (:229).)  Two
 * phases: gs_densify_count writes counters, the caller sizes the outputs
 * (n_out = 0, everything pruned: there is nothing to emit, and
 * gs_densify_emit refuses the NULL outputs an empty allocation has).
 *
 * Screen-space criterion (the 3DGS one; every field below is a trailing one,
 * all zero: the behaviour above, bit for bit).  With grad_accum / grad_denom
 * (the statistics gs_density_accumulate keeps) the gradient test reads
 *   g = grad_denom[i] > 0 ? grad_accum[i] / grad_denom[i] : 0
 * -- the mean over the views that saw i of the NDC-unit norm of the gradient
 * at its projected centre -- in place of |dL/dxyz_i|; a Gaussian no view saw
 * is never hot.  xyz_grad together with grad_accum, or grad_accum without
 * grad_denom, is GS_ERR_INVALID_ARG.  With GS_DENSIFY_PRUNE, max_radii given
 * and max_screen_radius > 0, big = max_radii[i] > max_screen_radius, and an
 * original that is big and not split produces no output: keep = !split and
 * alive and !big, clone = clone and alive and !big.  A split's children are
 * new and smaller: unaffected.  Split geometry, clone jitter, output order,
 * moment remap and counters are as above either way.
 *
 * AbsGS rule (trailing fields too, zero: the above bit for bit).  With
 * split_accum (the absolute statistic of gs_density_accumulate_abs) the split
 * test reads
 *   ga = grad_denom[i] > 0 ? split_accum[i] / grad_denom[i] : 0
 * against split_threshold -- split = ga > split_threshold and s > split_size *
 * scene_extent -- while the clone test keeps g against grad_threshold: large
 * Gaussians split on the absolute gradient, which their signed per-pixel
 * gradients cannot cancel, small ones clone on the signed one.  split_accum
 * without grad_accum / grad_denom is GS_ERR_INVALID_ARG.
 *
 * gs_density_accumulate adds one rendered view to those statistics, after
 * that view's backward: one launch, one thread per Gaussian, no atomics.  For
 * every g < n with vis[g] != 0, with W, H the rendered image's size,
 *   gx = (grad_sums ? grad_sums[g * GS_PAIR_GRAD_FLOATS + 0] : 0) + (g_means2d ? g_means2d[2g]     : 0)
 *   gy = (grad_sums ? grad_sums[g * GS_PAIR_GRAD_FLOATS + 1] : 0) + (g_means2d ? g_means2d[2g + 1] : 0)
 *   grad_accum[g] += sqrtf((0.5f W gx)^2 + (0.5f H gy)^2)
 *   denom[g]      += 1
 *   max_radii[g]   = fmaxf(max_radii[g], radii[g])
 * (0.5 W, 0.5 H: a per-pixel gradient in the NDC units the 3DGS threshold is
 * defined for).  grad_sums is what the blend backward's gather leaves -- the
 * blend's dL/dmeans2d in columns 0..1 -- or NULL for a frame without a blend
 * gradient; g_means2d is the caller's own cotangent on means2d, or NULL.  A
 * row with vis[g] == 0 is neither read nor written: its three values keep
 * their bits.  n == 0: GS_OK, nothing launched; a NULL required pointer or a
 * non-positive size: GS_ERR_INVALID_ARG before any HIP call. */
typedef struct gs_density_stats_args {
  int32_t n;
  int32_t image_width, image_height; /* gs_camera.image_width / image_height of the rendered view */
  const uint8_t *vis;                /* [n] the forward's visibility */
  const float *radii;                /* [n] the forward's radii */
  const float *grad_sums;            /* [n, GS_PAIR_GRAD_FLOATS], or NULL */
  const float *g_means2d;            /* [n, 2], or NULL */
  float *grad_accum, *denom, *max_radii; /* [n] each, read-modify-written where visible */
} gs_density_stats_args;
gs_status gs_density_accumulate(const gs_density_stats_args *a, gs_stream_t stream);
/* gs_density_accumulate with the absolute statistic: one launch in place of
 * that one (not after it).  stats' grad_accum, denom and max_radii get exactly
 * what gs_density_accumulate gives them, bit for bit, and for the same rows
 *   ax = (abs_sums ? abs_sums[2g]     : 0) + (g_means2d ? |g_means2d[2g]|     : 0)
 *   ay = (abs_sums ? abs_sums[2g + 1] : 0) + (g_means2d ? |g_means2d[2g + 1]| : 0)
 *   abs_accum[g] += sqrtf((0.5f W ax)^2 + (0.5f H ay)^2)
 * abs_sums is what gs_gather_abs_partials leaves (the colour pass's blend;
 * feature and distortion passes add to grad_sums only), or NULL for a frame
 * without a blend gradient.  A row with vis[g] == 0 is neither read nor
 * written.  Checks as gs_density_accumulate, and a NULL abs_accum with n > 0
 * is GS_ERR_INVALID_ARG. */
typedef struct gs_density_abs_args {
  gs_density_stats_args stats;       /* gs_density_accumulate's arguments */
  const float *abs_sums;             /* [n, 2], or NULL */
  float *abs_accum;                  /* [n], read-modify-written where visible */
} gs_density_abs_args;
gs_status gs_density_accumulate_abs(const gs_density_abs_args *a, gs_stream_t stream);

#define GS_DENSIFY_SPLIT 1
#define GS_DENSIFY_CLONE 2
#define GS_DENSIFY_PRUNE 4
typedef struct gs_model_arrays {
  float *xyz;           /* [n,3]   _xyz */
  float *features_dc;   /* [n,3]   _features_dc */
  float *features_rest; /* [n,rest_floats] _features_rest */
  float *scaling;       /* [n,3]   _scaling (log) */
  float *rotation;      /* [n,4]   _rotation */
  float *opacity;       /* [n]     _opacity (logit) */
} gs_model_arrays;
typedef struct gs_densify_args {
  int32_t n;
  int32_t rest_floats;
  gs_model_arrays in;             /* read only */
  const float *xyz_grad;          /* [n,3], or NULL: nothing is split or cloned (unless grad_accum is given) */
  float grad_threshold, scene_extent;
  float split_size, clone_size;   /* 0.03, 0.01 (gaussian_model.py:137,166) */
  float min_opacity;              /* 0.01 (optimizer.py:64) */
  int32_t flags;                  /* GS_DENSIFY_SPLIT | _CLONE | _PRUNE */
  uint64_t seed;                  /* clone jitter: counter-based normals, deterministic */
  gs_model_arrays adam_m_in, adam_v_in;   /* NULL members: not remapped */
  void *workspace;
  size_t workspace_bytes;
  uint32_t *counters;             /* [4]: kept, split children per side, clones, n_out */
  gs_model_arrays out, adam_m_out, adam_v_out;
  /* the screen-space criterion (above); all zero: |xyz_grad| and no radius prune */
  const float *grad_accum, *grad_denom; /* [n] each: the gradient test reads their quotient */
  const float *max_radii;         /* [n], or NULL */
  float max_screen_radius;        /* > 0 with max_radii and GS_DENSIFY_PRUNE: drop larger unsplit originals */
  /* AbsGS (above); both zero: split and clone read the same mean */
  const float *split_accum;       /* [n] gs_density_accumulate_abs' abs_accum, or NULL */
  float split_threshold;          /* the split test's threshold on split_accum / grad_denom */
} gs_densify_args;
size_t gs_densify_workspace_bytes(int32_t n);
gs_status gs_densify_count(const gs_densify_args *a, gs_stream_t stream);
gs_status gs_densify_emit(const gs_densify_args *a, gs_stream_t stream);

/* ---- MCMC density control (3DGS-MCMC, Kheradmand et al. 2024) -------------
 * The other family of density control: nothing is pruned and no gradient
 * threshold decides.  Dead Gaussians (opacity <= min_opacity) are moved onto
 * live ones drawn with probability proportional to their opacity, so that the
 * rendered image is preserved; new rows are added the same way up to a fixed
 * cap; and every iteration the positions get opacity-gated noise.  (Not in
 * the reference.)  All four entry points: one thread per item, no allocation,
 * no floating-point atomics; a NULL required pointer, a negative size or a
 * non-finite scalar is GS_ERR_INVALID_ARG before any HIP call; n == 0 or zero
 * samples is GS_OK with nothing launched.
 *
 * gs_mcmc_sample: weighted sampling with replacement, exact and reproducible.
 * cdf[i] is the inclusive prefix sum of non-negative integer weights
 * (total = cdf[n-1], read on the device).  With mix64 the splitmix64 finaliser
 * (z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;
 * z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31), sample j is
 *   h = mix64(seed ^ mix64(j)),  r = (h * total) >> 64,
 *   idx[j] = the smallest i with cdf[i] > r,   counts[idx[j]] += 1 (integer atomic)
 * so a row of weight 0 is never drawn.  counts is zeroed by the caller.
 * total == 0: GS_OK, nothing written (there is nothing to draw from). */
typedef struct gs_mcmc_sample_args {
  int32_t n;            /* rows of cdf and counts */
  int32_t num_samples;
  const int64_t *cdf;   /* [n] inclusive prefix sums, non-decreasing, cdf[n-1] < 2^63 */
  uint64_t seed;
  int32_t *idx;         /* [num_samples] out */
  int32_t *counts;      /* [n] in/out: += the times each row was drawn */
} gs_mcmc_sample_args;
gs_status gs_mcmc_sample(const gs_mcmc_sample_args *a, gs_stream_t stream);

/* gs_mcmc_relocate: the relocation (paper Eq. 9), in place, two launches.
 * Launch 1, per sample j with s = idx[j], in double from the fp32 inputs:
 *   R = min(counts[s] + 1, 51)
 *   o = min(sigmoid(opacity[s]), 1 - 2^-24)
 *   x = 1 - (1 - o)^(1/R)
 *   D = sum_{i=1..R} sum_{k=0..i-1} C(i-1, k) (-1)^k x^(k+1) / sqrt(k+1)
 *   opacity' = logit(clamp(x, min_opacity, 1 - 2^-24))
 *   scaling'[k] = scaling[s][k] + log(o / D)      (scaling[s][k] if D is not a positive finite number)
 * each rounded once to fp32 into workspace[j].  R == 1: x = o, D = o, the
 * scale unchanged.  Launch 2, per sample j: row dst[j] gets xyz, features_dc,
 * features_rest and rotation of row s bit for bit and opacity', scaling';
 * row s gets opacity', scaling' too; the rows s and dst[j] of every array
 * given in adam_m / adam_v become zero (NULL members are skipped).
 * Preconditions (the caller's; they make launch 2 free of races): the dst
 * rows are distinct, and no dst row is also sampled -- dead rows have weight
 * 0, appended rows lie past n.  idx[j] outside [0, n) or dst[j] outside
 * [0, rows) skips the sample.  min_opacity outside (0, 1): GS_ERR_INVALID_ARG. */
typedef struct gs_mcmc_relocate_args {
  int32_t n;                 /* rows that can be sampled: counts is [n], idx[j] < n */
  int32_t rows;              /* rows of params and the moments (>= n): dst[j] < rows */
  int32_t rest_floats;
  int32_t num_samples;
  gs_model_arrays params;    /* in place */
  gs_model_arrays adam_m, adam_v; /* in place; NULL members: not touched */
  const int32_t *idx;        /* [num_samples] gs_mcmc_sample's */
  const int32_t *counts;     /* [n] gs_mcmc_sample's */
  const int32_t *dst;        /* [num_samples] the rows that receive the copies */
  float min_opacity;
  void *workspace;           /* gs_mcmc_relocate_workspace_bytes(num_samples), 16-byte aligned */
  size_t workspace_bytes;
} gs_mcmc_relocate_args;
size_t gs_mcmc_relocate_workspace_bytes(int32_t num_samples);
gs_status gs_mcmc_relocate(const gs_mcmc_relocate_args *a, gs_stream_t stream);

/* gs_mcmc_noise: the per-iteration position noise, one streaming launch
 * (44 B read, 12 B written per Gaussian).  Per Gaussian i, in fp32:
 *   q = rotation[i] / max(|rotation[i]|, 1e-12),  Sigma = R(q) diag(exp(scaling[i])^2) R(q)^T
 *   o = sigmoid(opacity[i]),  gate = 1 / (1 + expf(-gate_steepness * (gate_midpoint - o)))
 *   eps[k] = the counter-based standard normal of (seed, i, k), k < 3 (the clone jitter's)
 *   xyz[i] += Sigma eps * (gate * scale)
 * scale = noise_lr * the xyz learning rate, formed by the caller.  Only xyz
 * is written.  scale == 0: GS_OK, nothing launched.  rotation is read as one
 * 16-byte vector per row and must be 16-byte aligned. */
typedef struct gs_mcmc_noise_args {
  int32_t n;
  float *xyz;            /* [n,3] in place */
  const float *scaling;  /* [n,3] log */
  const float *rotation; /* [n,4] */
  const float *opacity;  /* [n] logit */
  uint64_t seed;
  float scale;
  float gate_steepness;  /* 100 */
  float gate_midpoint;   /* 0.005 (1 - the paper's 0.995) */
} gs_mcmc_noise_args;
gs_status gs_mcmc_noise(const gs_mcmc_noise_args *a, gs_stream_t stream);

/* gs_mcmc_regularize: the gradients of
 *   lambda_opacity * mean(sigmoid(opacity)) + lambda_scale * mean(exp(scaling))
 * added to existing gradient buffers, with o = sigmoid(opacity[i]):
 *   d_opacity[i]    += (lambda_opacity / n) * o * (1 - o)
 *   d_scaling[i][k] += (lambda_scale / (3 n)) * exp(scaling[i][k])
 * (the two factors formed in double and rounded to fp32 once).  A NULL
 * gradient pointer skips that term; both NULL: nothing launched. */
typedef struct gs_mcmc_regularize_args {
  int32_t n;
  const float *opacity;  /* [n] logit */
  const float *scaling;  /* [n,3] log */
  float *d_opacity;      /* [n], or NULL */
  float *d_scaling;      /* [n,3], or NULL */
  float lambda_opacity, lambda_scale;
} gs_mcmc_regularize_args;
gs_status gs_mcmc_regularize(const gs_mcmc_regularize_args *a, gs_stream_t stream);

/* ---- 3D smoothing filter (Mip-Splatting, Yu et al. 2024, Sec. 4.1) ---------
 * The other half of the anti-aliased mode (gs_screen_filter is the 2D half):
 * every Gaussian is convolved in world space with an isotropic Gaussian of
 * standard deviation f = sqrt(variance) / nu, nu the highest sampling rate
 * (pixels per world unit, focal / depth) any training camera saw it at, so
 * that no splat is thinner than what the training views could resolve.  The
 * filter is a per-Gaussian map in front of the projection,
 *   (scaling, opacity logit, f) -> (scaling', opacity'),
 * whose outputs gs_gaussians takes as they are (scaling, opacity with
 * opacity_is_logit = 0); the projection kernels do not know of it.  Stream
 * ordered, one thread per Gaussian, no allocation, no atomics; every check
 * below returns GS_ERR_INVALID_ARG before any HIP call; n == 0 is GS_OK with
 * nothing launched. */
#define GS_FILTER3D_CAMERA_FLOATS 18

/* gs_filter3d_accumulate: the sampling-rate pass over num_cameras cameras in
 * one launch (each position is read once).  A camera row is
 *   {view[12] (row-major 3x4, world -> camera), fx, fy, cx, cy, W, H}.
 * Per Gaussian and camera, in double from the fp32 inputs: (X, Y, Z) = R x + t;
 * the camera sees the Gaussian iff Z > near and
 *   -margin W <= fx X / Z + cx <= (1 + margin) W,
 *   -margin H <= fy Y / Z + cy <= (1 + margin) H;
 * its rate is max(fx, fy) / Z.  Then
 *   max_rate[g] = fmaxf(max_rate[g], (float)(max over the seeing cameras)),
 * and a Gaussian no camera sees keeps its value.  num_cameras == 0: GS_OK,
 * nothing launched. */
typedef struct gs_filter3d_rate_args {
  int32_t n;
  const float *xyz;      /* [n, xyz_stride] */
  int64_t xyz_stride;    /* floats between rows, >= 3 */
  const float *cameras;  /* device [num_cameras, GS_FILTER3D_CAMERA_FLOATS] */
  int32_t num_cameras;
  float near;            /* finite, > 0 (Mip-Splatting: 0.2) */
  float margin;          /* finite, >= 0 (Mip-Splatting: 0.15) */
  float *max_rate;       /* [n] in/out */
} gs_filter3d_rate_args;
gs_status gs_filter3d_accumulate(const gs_filter3d_rate_args *a, gs_stream_t stream);

/* gs_filter3d_forward / gs_filter3d_backward: the map and its gradient.
 *   s'_k = 1/2 log(exp(2 s_k) + f^2)
 *   o'   = sigmoid(o) sqrt(prod_k exp(2 s_k) / (exp(2 s_k) + f^2))
 * (o' a probability), computed without overflow as, L = log f,
 * d_k = 2 (s_k - L) -- both formed in double from the fp32 inputs and rounded
 * to fp32 once -- and r_k = sigmoid(d_k), in fp32:
 *   s'_k = max(s_k, L) + 1/2 log1pf(expf(-|d_k|)),  coef = sqrtf(r_0 r_1 r_2),
 *   o' = sigmoid(o) coef.
 * A row with f == 0 copies s bit for bit and writes sigmoid(o).  The backward
 * stores (does not add)
 *   d_scaling_k = g_scaling_out_k r_k + g_opacity_out o' (1 - r_k)
 *   d_opacity   = g_opacity_out coef sigmoid(o) (1 - sigmoid(o))
 * with 1 - r_k formed as sigmoid(-d_k); f carries no gradient; f == 0:
 * d_scaling = g_scaling_out bit for bit.  All rows are dense.  The forward
 * reads the first five pointers, the backward all but the two outputs. */
typedef struct gs_filter3d_args {
  int32_t n;
  const float *scaling;   /* [n,3] log */
  const float *opacity;   /* [n] logit */
  const float *filter;    /* [n] f >= 0, world units */
  float *scaling_out;     /* [n,3] log (forward) */
  float *opacity_out;     /* [n] probability (forward) */
  const float *g_scaling_out; /* [n,3] (backward) */
  const float *g_opacity_out; /* [n] (backward) */
  float *d_scaling;       /* [n,3] (backward) */
  float *d_opacity;       /* [n] (backward) */
} gs_filter3d_args;
gs_status gs_filter3d_forward(const gs_filter3d_args *a, gs_stream_t stream);
gs_status gs_filter3d_backward(const gs_filter3d_args *a, gs_stream_t stream);

/* ---- Normal consistency (2DGS, Huang et al. 2024, Sec. 5) ------------------
 * The other half of the geometry regularisation, next to the depth distortion:
 * each Gaussian's normal, composited per pixel by the feature pass
 * (N_r = sum_i c_i n_i), should agree with the normal of the surface the depth
 * map implies.  Two per-Gaussian kernels make the normals and their gradient,
 * two per-pixel kernels the error and its gradient; the blend in between is
 * gs_blend_features_*.  Stream ordered, no allocation, no atomics, no host
 * sync, the same bits every run; every check below returns
 * GS_ERR_INVALID_ARG before any HIP call. */

/* gs_gaussian_normals_forward / _backward: one thread per Gaussian.
 *   k   = argmin_k scaling[k], the first among equals (the flat axis)
 *   q^  = q / max(|q|, 1e-12), q = rotation row (w, x, y, z), un-normalised
 *   n_w = column k of R(q^)               (gs_gaussians' rotation matrix)
 *   n_c = Rv n_w,  p_c = Rv xyz + t       (view = [Rv | t], row-major 3x4)
 *   normals = n_c . p_c > 0 ? -n_c : n_c  (faces the camera; an exact 0 keeps the sign)
 * computed in double from the fp32 inputs and rounded once.  The backward
 * stores (does not add) d_rotation from g_normals through the flip sign, Rv,
 * column k and the normalisation; the axis choice and the flip are piecewise
 * constant, so scaling, xyz and the view receive nothing.  n == 0 is GS_OK
 * with nothing launched.  The forward reads rotation, scaling, xyz, view and
 * writes normals; the backward reads g_normals too and writes d_rotation. */
typedef struct gs_gaussian_normals_args {
  int32_t n;
  const float *rotation;  /* [n,4] raw (w, x, y, z) */
  const float *scaling;   /* [n,3] log */
  const float *xyz;       /* [n, xyz_stride] */
  int64_t xyz_stride;     /* floats between rows, >= 3 */
  float view[12];         /* row-major 3x4, world -> camera */
  float *normals;         /* [n,3] camera space (forward) */
  const float *g_normals; /* [n,3] (backward) */
  float *d_rotation;      /* [n,4] (backward) */
} gs_gaussian_normals_args;
gs_status gs_gaussian_normals_forward(const gs_gaussian_normals_args *a, gs_stream_t stream);
gs_status gs_gaussian_normals_backward(const gs_gaussian_normals_args *a, gs_stream_t stream);

/* gs_normal_consistency_forward / _backward: one thread per pixel.  With the
 * renderer's conventions (integer pixel coordinates, y_pix = -fy Y / Z + cy),
 * N = normals, D = depth, A = alpha:
 *   r(x,y) = ((x - cx) / fx, -(y - cy) / fy, 1),  P = D r
 *   interior pixels (1 <= x <= W-2, 1 <= y <= H-2):
 *     dx = P(x+1,y) - P(x-1,y),  dy = P(x,y+1) - P(x,y-1),  m = dx x dy
 *     n_d = m / |m| where |m| is finite and > 1e-20, else 0
 *   border pixels: n_d = 0
 *   error = 1 - A (N . n_d)
 * (2DGS's 1 - sum rend_normal * surf_normal * alpha.detach(); dx x dy faces
 * the camera: negative z for a fronto-parallel plane).  In fp32, the
 * differences formed as (D+ - D-) r + (D+ + D-) (1/fx, 0, 0) and
 * (D+ - D-) r + (D+ + D-) (0, -1/fy, 0).  surface_normals receives n_d, or is
 * NULL.  The backward stores, from g_error,
 *   d_normals = -A g_error n_d
 *   g_n = -A g_error N,  g_m = (g_n - n_d (n_d . g_n)) / |m|  (0 where n_d is 0)
 *   g_dx = dy x g_m,  g_dy = g_m x dx
 *   d_depth(x,y) = r(x,y) . [g_dx(x-1,y) - g_dx(x+1,y) + g_dy(x,y-1) - g_dy(x,y+1)]
 * (0 for a neighbour that is not interior) as a gather; alpha is a weight and
 * receives no gradient.  width, height >= 1 (height <= 262140); fx, fy finite
 * and not 0; cx, cy finite. */
typedef struct gs_normal_consistency_args {
  int32_t width, height;
  float fx, fy, cx, cy;
  const float *normals;   /* [3,H,W] */
  const float *depth;     /* [H,W] */
  const float *alpha;     /* [H,W] */
  float *error;           /* [H,W] (forward) */
  float *surface_normals; /* [3,H,W], or NULL (forward) */
  const float *g_error;   /* [H,W] (backward) */
  float *d_normals;       /* [3,H,W] (backward) */
  float *d_depth;         /* [H,W] (backward) */
} gs_normal_consistency_args;
gs_status gs_normal_consistency_forward(const gs_normal_consistency_args *a, gs_stream_t stream);
gs_status gs_normal_consistency_backward(const gs_normal_consistency_args *a, gs_stream_t stream);

/* ---- Frame entry points: the stages above in one call per direction -------
 * gs_render_forward runs what GaussianRenderer.render does (renderer.py:31-114)
 * -- projection + culling, depth sort, binning, tile sort, ranges, blend --
 * and gs_render_backward its autograd backward, over two caller-owned
 * workspaces the library lays out: a frame workspace (per Gaussian and per
 * pixel, gs_frame_workspace_bytes) and a tile workspace (per list entry, for up
 * to `capacity` entries, gs_tile_workspace_bytes).  The host reads the
 * frame's counts (M, T, the visible depth range) back once, inside
 * gs_render_forward, by polling a pinned buffer the count writes through its
 * device address.  Both workspaces must stay untouched from the forward to
 * its backward. */
typedef struct gs_frame_buffers {
  void *frame_ws;        /* gs_frame_workspace_bytes(n, W, H, tile_size) */
  size_t frame_ws_bytes;
  void *tile_ws;         /* gs_tile_workspace_bytes(capacity, tiles, live_cells, flag_groups) */
  size_t tile_ws_bytes;
  int64_t capacity;      /* list entries the tile workspace holds */
  int32_t live_cells;    /* cells of the liveness bitmap (gs_tile_quads), or 0: none (a memory budget) */
  int32_t flag_groups;   /* slot flags per entry: the backward's partial groups per batch */
} gs_frame_buffers;
size_t gs_frame_workspace_bytes(int32_t n, int32_t width, int32_t height, int32_t tile_size);
size_t gs_tile_workspace_bytes(int64_t capacity, int32_t num_tiles, int32_t live_cells, int32_t flag_groups);

typedef struct gs_render_fwd_args {
  gs_camera cam;
  gs_gaussians g;
  float *means2d, *conics, *radii; /* outputs, as gs_project_args */
  uint8_t *vis;
  float *image, *alpha, *depth;    /* outputs, as gs_blend_fwd_args */
  gs_frame_buffers fb;
  uint32_t key_base;               /* the depth-key window (gs_project_args) */
  int32_t key_bits;
  int32_t depth_sort_msd;          /* 1: gs_depth_sort_msd for windows of 9..31 bits */
  int32_t zero_slot_flags;         /* a backward follows: clear its slot flags [T, flag_groups] */
  uint32_t *host_counters_dev;     /* pinned [8] u32: device address (gs_bin_args.host_counters) */
  volatile uint32_t *host_counters_host; /* ... and host address of the same buffer */
  uint32_t host_seq;               /* this frame's sequence word (never the previous frame's) */
  uint32_t *pair_counts;           /* optional, gs_blend_fwd_args.pair_counts */
  uint32_t *pix_neval;             /* optional, gs_blend_fwd_args.pix_neval */
  int32_t resume;                  /* 1: continue after GS_NEED_CAPACITY, with a tile workspace of >= T */
  int32_t poll_timeout_ms;         /* the counter poll's patience before it synchronises the stream and
                                      looks once more (0: 10 s) */
  /* Device-resident frame (device_counts = 1): no host read-back at all.  The
   * count's status (GS_FRAME_*) and T stay on the device: the tile sort, the
   * ranges and the blend are launched for `capacity` entries (needs a tile
   * workspace) and read T themselves; a failed frame is drawn with empty
   * lists -- the background once, zero alpha and depth -- and flagged in
   * counters[4] (and *step_flags).  The call returns
   * GS_OK with M, T unknown; the host reads (M, T, depth range, seq, status)
   * from the pinned counters whenever it likes.  For graph capture. */
  int32_t device_counts;
  uint32_t *step_flags;            /* optional, gs_bin_args.step_flags */
  uint32_t *frame_seq;             /* optional, gs_bin_args.frame_seq */
  /* results (and state for resume / the backward) */
  int32_t M, T;
  uint32_t depth_min_bits, depth_max_bits; /* counters[2..3] */
  int32_t depth_alt, tile_alt;
  gs_screen_filter filter;         /* (input) passed to gs_project_forward; all zero: none */
} gs_render_fwd_args;
/* GS_OK; M == 0: nothing drawn (renderer.py:74-83's background image is the
 * caller's); GS_NEED_CAPACITY / GS_RETRY_FULL_KEYS: see gs_status. */
gs_status gs_render_forward(gs_render_fwd_args *a, gs_stream_t stream);

typedef struct gs_render_bwd_args {
  gs_camera cam;
  gs_gaussians g;
  gs_frame_buffers fb;             /* the forward's */
  int32_t M, T, tile_alt;          /* the forward's results */
  const float *means2d, *conics;   /* the forward's outputs */
  const uint8_t *vis;
  const float *image, *alpha, *depth; /* the forward's outputs, unmodified (the blend backward reads them) */
  const float *g_image, *g_alpha, *g_depth; /* pixel cotangents (g_image NULL: none) */
  const float *g_means2d, *g_conics;        /* optional */
  float *pair_grads;               /* [T * fb.flag_groups, GS_PARTIAL_STRIDE] scratch */
  int32_t flags_zeroed;            /* the forward cleared the slot flags (zero_slot_flags) */
  int32_t project;                 /* 1: also run gs_project_backward over every Gaussian */
  float *d_xyz, *d_cov3d, *d_scaling, *d_rotation, *d_color_logits, *d_opacity, *d_sh_rest; /* as gs_project_bwd_args */
  float *grad_sums;                /* result: [n, 10] gathered sums in the frame workspace (for a
                                      caller's own gs_project_backward, e.g. per row range) */
  void *blend_events[2];           /* optional hipEvent_t pair, recorded on the stream right before and
                                      after the blend backward launch(es): its time alone (profiling) */
  int32_t device_counts;           /* the forward was device-resident: M, T are not read; pair_grads holds
                                      capacity * flag_groups partials (a failed frame gathers zero slots) */
  const gs_adam_args *fused_adam;  /* with project = 1: gs_project_backward_adam with these tensors (no
                                      d_* written), or NULL: the plain projection backward */
  gs_screen_filter filter;         /* the forward's, passed to the projection backward */
} gs_render_bwd_args;
gs_status gs_render_backward(gs_render_bwd_args *a, gs_stream_t stream);
/* Byte offsets of the buffers inside the two workspaces (for diagnostics and
 * tests that inspect a frame): frame -- records, rects, depth keys [2,n],
 * depth ids [2,n], key_minmax, counters, sort workspace, binning workspace,
 * pair_offset, tile ranges, pixel clamp flags, per-cell evaluated entries
 * (gs_blend_fwd_args.pix_flags / cell_neval), grad_sums, total; tile -- tile
 * keys (two halves), Gaussian ids (two halves), sort workspace, liveness
 * bitmap, slot flags, total, liveness words per cell. */
void gs_frame_offsets(int32_t n, int32_t width, int32_t height, int32_t tile_size, size_t out[14]);
void gs_tile_offsets(int64_t capacity, int32_t num_tiles, int32_t live_cells, int32_t flag_groups, size_t out[9]);

/* ---- Bilateral grid (Wang et al., "Bilateral Guided Radiance Field
 * Processing", SIGGRAPH 2024; HDRNet's slicing; gsplat's use_bilateral_grid) ---
 * Appearance compensation: one small learnable grid of affine colour
 * transforms per training image, sliced per pixel and applied to the render
 * before the photometric loss, held smooth by a total-variation term.  It sits
 * wholly behind the rendered image.  Stream ordered, no allocation, no atomics,
 * no host sync, the same bits every run; every check below returns
 * GS_ERR_INVALID_ARG before any HIP call.
 *
 * A grid G is [12, L, Gh, Gw] fp32, channel 4c + k entry (c, k) of a 3x4 affine
 * matrix; 2 <= L <= GS_BILAGRID_MAX_L, 2 <= Gh, Gw <= GS_BILAGRID_MAX_XY.  For
 * pixel (x, y) of the [3, H, W] image rgb = (r, g, b), in fp32:
 *   u = (x + 0.5) / W * (Gw - 1),  v = (y + 0.5) / H * (Gh - 1)
 *   gray = (0.299 r + 0.587 g) + 0.114 b,  z = clamp(gray, 0, 1) * (L - 1)
 *   along each axis  i0 = clamp(floor(t), 0, n - 2),  f = t - i0
 *   A = trilinear(G; u, v, z) as nested lerps a0 + f (a1 - a0): x, then y, then z
 *   out[c] = ((A[c,0] r + A[c,1] g) + A[c,2] b) + A[c,3]
 * (torch's 5-D grid_sample, bilinear, border padding, align_corners; a grid
 * constant over its nodes is sliced exactly, the identity grid returns the
 * image bit for bit).  The backward stores, from g_out [3, H, W],
 *   d_grid[4c+k, node] = sum over the pixels of  w_x w_y w_z  g_out[c] (r, g, b, 1)[k]
 *     with each axis' weights 1 - f at i0 and f at i0 + 1 -- every node is
 *     written, a node no pixel touches gets an exact 0 -- and
 *   d_rgb[k] = sum_c g_out[c] A[c,k]
 *              + coef[k] (L - 1) [0 < gray < 1] sum_c g_out[c] (dA/dz)[c,:] . (r, g, b, 1)
 *     with coef = (0.299, 0.587, 0.114) and dA/dz = a1 - a0 of the z lerp (no
 *     gradient through the guidance where gray is clamped; u, v are constants).
 * The forward is one launch of one thread per pixel; the backward two: d_rgb
 * per pixel, and d_grid as a gather -- one workgroup per node column (gx, gy)
 * walks the pixels of the column's two-cell footprint, every thread keeps the
 * column's L x 12 sums in registers, and the workgroup adds them in a fixed
 * order.  The per-pixel kernels keep the grid in LDS when it fits 112 KiB (the
 * default shape takes 96) and read it from memory otherwise.  width, height
 * >= 1 (height <= 262140, at most 2^30 tiles of 64 x 16 pixels). */
#define GS_BILAGRID_CHANNELS 12
#define GS_BILAGRID_MAX_L 16
#define GS_BILAGRID_MAX_XY 64
typedef struct gs_bilagrid_slice_args {
  int32_t width, height;          /* the image */
  int32_t grid_w, grid_h, grid_l; /* Gw, Gh, L */
  const float *grid;              /* [12, L, Gh, Gw] */
  const float *rgb;               /* [3,H,W] */
  float *out;                     /* [3,H,W] (forward) */
  const float *g_out;             /* [3,H,W] (backward) */
  float *d_rgb;                   /* [3,H,W] (backward) */
  float *d_grid;                  /* [12, L, Gh, Gw] (backward) */
} gs_bilagrid_slice_args;
gs_status gs_bilagrid_slice_forward(const gs_bilagrid_slice_args *a, gs_stream_t stream);
gs_status gs_bilagrid_slice_backward(const gs_bilagrid_slice_args *a, gs_stream_t stream);

/* gs_bilagrid_tv: the total variation of one grid and its gradient, one launch
 * of one workgroup (the sums in double, in a fixed order):
 *   tv = mean_x-pairs (G[.., x+1] - G[.., x])^2 + mean_y-pairs (..)^2 + mean_z-pairs (..)^2
 * each mean over that axis' own neighbour pairs and all 12 channels, and
 *   d_grid[n] = sum over the axes of (2 / pairs_axis) ((G[n] - G[n - 1]) - (G[n + 1] - G[n]))
 * (a difference that has no neighbour is 0).  tv is one float. */
typedef struct gs_bilagrid_tv_args {
  int32_t grid_w, grid_h, grid_l;
  const float *grid; /* [12, L, Gh, Gw] */
  float *tv;         /* [1] */
  float *d_grid;     /* [12, L, Gh, Gw]: d tv / d grid */
} gs_bilagrid_tv_args;
gs_status gs_bilagrid_tv(const gs_bilagrid_tv_args *a, gs_stream_t stream);

/* ---- TSDF fusion and mesh extraction (KinectFusion's / Open3D's z-projective
 * running mean, which 2DGS's mesh extraction uses; surface nets, Gibson 1998) --
 * Rendered depth maps are fused into a truncated signed distance volume and a
 * triangle mesh is extracted from it.  Stand-alone: nothing here is part of a
 * render or a training step.  Stream ordered, no allocation, no atomics, no
 * host sync, the same bits every run; every check below returns before any HIP
 * call: GS_ERR_INVALID_ARG for a null pointer, a dimension below 1 or a bad
 * scalar, GS_ERR_UNSUPPORTED for a volume of 2^31 nodes or more.
 *
 * A volume is nx x ny x nz samples at the nodes p_ijk = origin + h (i, j, k),
 * stored [nz, ny, nx] with x fastest: tsdf (initially 1), weight (initially 0)
 * and optionally color [3, nz, ny, nx] (initially 0), all fp32. */
typedef struct gs_tsdf_volume {
  int32_t nx, ny, nz;
  float origin[3];
  float voxel_size; /* h, finite and > 0 */
  float *tsdf;      /* [nz,ny,nx] */
  float *weight;    /* [nz,ny,nx] */
  float *color;     /* [3,nz,ny,nx], or NULL */
} gs_tsdf_volume;

/* gs_tsdf_integrate fuses num_views >= 1 views of one size in one launch.  A
 * camera row is {view[12], fx, fy, cx, cy}: gs_camera's values, the first 16
 * floats of a gs_filter3d_rate_args row.  One thread owns a node and visits
 * the views in table order, in fp32:
 *   (X, Y, Z) = R p + t, each ((r0 x + r1 y) + r2 z) + t;  skip unless Z > near
 *   px = (fx X) / Z + cx,  py = (-fy Y) / Z + cy     (the projection's convention)
 *   u = floor(px + 0.5), v = floor(py + 0.5);  skip outside [0, W) x [0, H)
 *   d = depth[v, u];  skip unless d > 0 (a NaN skips), if d > depth_max, and
 *   if alpha is given and alpha[v, u] < alpha_min
 *   s = d - Z;  skip if s < -trunc;  tau = min(1, s / trunc)
 *   w' = w + 1;  tsdf = (tsdf w + tau) / w';  color_c = (color_c w + image[c, v, u]) / w'
 *   (the colour with both a colour volume and an image);  w = w'
 * The node stays in registers over the views: num_views views in one launch
 * give the bits of num_views launches of one view each, in order, with one
 * read and one write of the volume.  A node no view updates is neither read
 * nor stored to.  near and trunc finite and > 0; alpha_min and depth_max not
 * NaN (depth_max may be +inf). */
#define GS_TSDF_CAMERA_FLOATS 16
typedef struct gs_tsdf_integrate_args {
  gs_tsdf_volume vol;
  int32_t num_views, width, height;
  const float *cameras; /* [V, GS_TSDF_CAMERA_FLOATS], on the device */
  const float *depth;   /* [V,H,W] */
  const float *alpha;   /* [V,H,W], or NULL */
  const float *image;   /* [V,3,H,W], or NULL */
  float near, trunc, alpha_min, depth_max;
} gs_tsdf_integrate_args;
gs_status gs_tsdf_integrate(const gs_tsdf_integrate_args *a, gs_stream_t stream);

/* Surface nets.  Cell (i, j, k), 0 <= i < nx - 1 and likewise j, k, has the 8
 * nodes (i..i+1, j..j+1, k..k+1) as corners.  A node is inside iff tsdf < 0; a
 * cell is valid iff all 8 corners have weight >= min_weight, and active iff it
 * is valid and its corners are not all on one side.  Every such test reads the
 * stored fp32 values.
 *
 * gs_mesh_classify writes, per cell, cell_active (0 / 1), and per node the
 * number of triangles its three edges emit (node_tris: 0, 2, 4 or 6) and their
 * 3-bit mask (node_mask, bit a for the edge n -> n + e_a).  With (a, b, c)
 * cyclic -- x: (y, z), y: (z, x), z: (x, y) -- edge a of node n emits iff its
 * ends differ in side and the four cells around it, c00 = n - e_b - e_c,
 * c10 = n - e_c, c11 = n and c01 = n - e_b, all exist and are valid.  One
 * workgroup classifies a 32 x 8 x 4 tile of nodes from an LDS image of the
 * tile's side and validity bits with a one-node apron.
 *
 * The caller forms the inclusive prefix sums of cell_active and node_tris
 * (int32) and reads the two totals; gs_mesh_emit then writes
 *   vertices[r] of the active cell of rank r (linear cell order, i fastest):
 *     over the cell's 12 edges -- the four x edges, then y, then z, within a
 *     group by the other two offsets in lexicographic order -- each edge whose
 *     ends a, b differ in side crosses at q = a + f (b - a), f = f_a / (f_a - f_b),
 *     in node units relative to the cell; the vertex is
 *     origin + h ((i, j, k) + mean q), its colour the mean of c_a + f (c_b - c_a);
 *   faces: per node in linear order, per set mask bit in the order x, y, z, the
 *     triangles (c00, c10, c11), (c00, c11, c01) of the cells' ranks when n is
 *     inside -- the normal along +a, from inside to outside -- and with the
 *     last two indices of each swapped when n is outside.
 * num_vertices or num_faces 0: that array is not written. */
typedef struct gs_mesh_args {
  gs_tsdf_volume vol;         /* read only here */
  float min_weight;           /* classify; not NaN */
  uint8_t *cell_active;       /* [nz-1,ny-1,nx-1] (may be NULL when there is no cell) */
  uint8_t *node_tris;         /* [nz,ny,nx] */
  uint8_t *node_mask;         /* [nz,ny,nx] */
  const int32_t *cell_rank;   /* emit: inclusive prefix sum of cell_active */
  const int32_t *node_faces;  /* emit: inclusive prefix sum of node_tris */
  int32_t num_vertices, num_faces; /* emit: the two totals */
  float *vertices;            /* emit: [num_vertices, 3] */
  float *colors;              /* emit: [num_vertices, 3], or NULL; needs vol.color */
  int32_t *faces;             /* emit: [num_faces, 3] */
} gs_mesh_args;
gs_status gs_mesh_classify(const gs_mesh_args *a, gs_stream_t stream);
gs_status gs_mesh_emit(const gs_mesh_args *a, gs_stream_t stream);

/* ---- k-nearest neighbours (simple_knn's distCUDA2: the start-up scale of
 * 3DGS and its descendants) -------------------------------------------------
 * Exact k-NN of every point of a cloud among the others.  Stand-alone, stream
 * ordered, no allocation, no atomics, no host read: a fixed launch sequence.
 *
 * The result is defined apart from the search.  d2(a, b) is
 * ((dx dx) + (dy dy)) + (dz dz) of the fp32 differences, in that order,
 * unfused -- one device function, the only place a distance is computed.  Row
 * i of the output is the k smallest pairs (d2(p_i, p_j), j), j != i, in
 * lexicographic order: equal distances resolve to the smaller row, and a
 * duplicate of p_i at another row is a neighbour at distance 0.  With fewer
 * than k other points the row is padded with +inf / -1.  mean_dist2[i] is the
 * sum of the min(k, n - 1) distances found, ascending, in fp32, divided by
 * their count (0 when n == 1).  So the bits do not depend on the run, the
 * rank or the order of the input rows.
 *
 * The search: Morton order over the cloud's bounding box (30-bit keys, the
 * device radix sort), boxes of 256 consecutive points with their AABBs, one
 * workgroup per query box and one query per lane, the best K = 4, 8 or 16
 * (the smallest >= k) in registers.  A box is passed over when its AABB's
 * distance to the query box's AABB is strictly above the largest k-th best of
 * the workgroup's queries, a query passes a staged box over when its own
 * distance to the AABB is strictly above its own k-th best.  Both bounds are
 * d2 of per-axis gaps that are no larger than the difference to any point of
 * the box, and fp32 subtraction, squaring and adding are monotone: a bound is
 * <= the computed d2 of every pair it stands for, with no epsilon, and on
 * equality the box is visited.
 *
 * Checks, before any HIP call: a NULL struct, k outside 1..GS_KNN_MAX_K,
 * n < 0, all three outputs NULL, and for n > 0 NULL points or a workspace
 * that is NULL, not 16-byte aligned or smaller than gs_knn_workspace_bytes(n):
 * GS_ERR_INVALID_ARG.  n > 2^30: GS_ERR_UNSUPPORTED (gs_knn_workspace_bytes
 * then returns 0, as for n <= 0).  n == 0: GS_OK, nothing launched.
 * Coordinates must be finite. */
#define GS_KNN_MAX_K 16
typedef struct gs_knn_args {
  int32_t n, k;        /* 1 <= k <= GS_KNN_MAX_K */
  const float *points; /* [n,3] */
  float *dist2;        /* [n,k] ascending; +inf where a point has fewer than k neighbours; may be NULL */
  int32_t *index;      /* [n,k] neighbour rows; -1 where none; may be NULL */
  float *mean_dist2;   /* [n] mean of the min(k, n-1) distances found (0 if n == 1); may be NULL */
  void *workspace;
  size_t workspace_bytes;
} gs_knn_args;
size_t gs_knn_workspace_bytes(int32_t n);
gs_status gs_knn(const gs_knn_args *a, gs_stream_t stream);

/* ---- misc --------------------------------------------------------------- */
int32_t gs_abi_version(void);
const char *gs_last_error(void);

#ifdef __cplusplus
}
#endif
#endif /* GSPLAT_MI355X_H */
