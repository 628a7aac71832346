"""Device pipeline + autograd for the render path.

One `render` = the reference's four stages (renderer.py:31-114):
  gs_project_forward   _project_gaussians_3d_to_2d + _frustum_culling
  gs_radix_sort_pairs  _sort_gaussians_by_depth (32-bit depth keys)
  gs_bin_count/emit    tile binning in depth order  (_tile_rasterization :263-298)
  gs_radix_sort_pairs  stable sort of the entries by tile id
  gs_tile_ranges       per-tile lists
  gs_blend_forward     per-pixel compositing        (:273-367)
and the backward: gs_blend_backward + gs_project_backward, then, when the
render was given a DensityStats, one gs_density_accumulate.

All buffers are torch tensors from the caching allocator; the HIP library
never allocates.  One host synchronisation per forward reads the visible
count M and the tile-touch count T (needed to size the entry buffers, and
for the reference's `vis_mask.sum() == 0` early return, renderer.py:74-83).
"""
from __future__ import annotations

import ctypes as C
import math
import os
import threading
import time
from dataclasses import dataclass
from typing import Optional, Tuple

import torch

from . import _native as N


@dataclass
class CameraParams:
    """Host-side scalars of one view, as renderer.py:140-152 derives them."""
    image_width: int
    image_height: int
    fx: float
    fy: float
    cx: float
    cy: float
    view: Tuple[float, ...]  # 12 floats, rows 0..2 of the W2C matrix
    bg: Tuple[float, float, float]
    radius_min: float = 0.01
    radius_max: float = 50.0
    tile_size: int = N.GS_DEFAULT_TILE  # GaussianRenderer(tile_size) (renderer.py:24,261-264)
    # the screen-space low-pass filter (gs_screen_filter; not in the reference): cov2d + screen_filter I
    # (px^2, 0 = off), and with filter_compensate the opacity scaled so that a splat keeps its energy
    screen_filter: float = 0.0
    filter_compensate: bool = True

    def __post_init__(self):
        check_screen_filter(self.screen_filter)

    @property
    def tiles_x(self) -> int:
        return (self.image_width + self.tile_size - 1) // self.tile_size

    @property
    def tiles_y(self) -> int:
        return (self.image_height + self.tile_size - 1) // self.tile_size

    @property
    def cells(self) -> int:
        """8x8 pixel cells per tile (gs_tile_quads): 4 at the default 16."""
        q = (self.tile_size + N.GS_QUAD - 1) // N.GS_QUAD
        return q * q

    @property
    def groups(self) -> int:
        """Gradient partials a one-batch blend backward writes per list entry
        (gs_partial_groups): one per 8x8 cell, 4 at the default tile.  Tiles
        of many cells may replay them in batches (frame_groups)."""
        return _partial_groups(self.tile_size)

    def frame_groups(self, entries: int) -> int:
        """Partials per entry of one backward batch for a frame of `entries`
        list entries: the combined default tile's one, else cell_batch."""
        return self.groups if self.groups < self.cells else cell_batch(self.cells, entries)

    def to_struct(self) -> N.GsCamera:
        """The ABI camera (cached per distinct value set: building it costs
        ~5-10 us of host time per frame; callers copy it into their
        argument structs and never modify it)."""
        key = (self.image_width, self.image_height, self.fx, self.fy, self.cx, self.cy, self.view, self.bg,
               self.radius_min, self.radius_max, self.tile_size, self.screen_filter, self.filter_compensate)
        c = _CAM_STRUCTS.get(key)
        if c is None:
            if len(_CAM_STRUCTS) >= 4096:
                _CAM_STRUCTS.clear()
            c = _CAM_STRUCTS[key] = self._build_struct()
        return c

    def filter_struct(self) -> N.GsScreenFilter:
        """The ABI filter for the trailing field of the projection's and the
        frame entry points' arguments (all zero when off)."""
        s = float(self.screen_filter)
        return N.GsScreenFilter(s, 1 if self.filter_compensate else 0) if s > 0.0 else _NO_FILTER

    def _build_struct(self) -> N.GsCamera:
        c = N.GsCamera()
        c.image_width, c.image_height = int(self.image_width), int(self.image_height)
        c.fx, c.fy, c.cx, c.cy = self.fx, self.fy, self.cx, self.cy
        c.view = (C.c_float * 12)(*self.view)
        c.radius_min, c.radius_max = self.radius_min, self.radius_max
        c.bg = (C.c_float * 3)(*self.bg)
        c.tile_size = int(self.tile_size)
        c.campos = (C.c_float * 3)(*self.campos)
        return c

    @property
    def campos(self) -> Tuple[float, float, float]:
        """Camera centre in world coordinates, -R^T t of the W2C view (the SH
        view direction's origin)."""
        v = self.view
        R = ((v[0], v[1], v[2]), (v[4], v[5], v[6]), (v[8], v[9], v[10]))
        t = (v[3], v[7], v[11])
        return tuple(-(R[0][j] * t[0] + R[1][j] * t[1] + R[2][j] * t[2]) for j in range(3))


def check_screen_filter(variance) -> None:
    """ValueError for a screen filter variance no render can use (negative, NaN or infinite)."""
    v = float(variance)
    if not (v >= 0.0 and math.isfinite(v)):
        raise ValueError(f"screen_filter must be a finite variance >= 0 (px^2), got {variance!r}")


_NO_FILTER = N.GsScreenFilter()  # (shared, never modified: callers copy it into their argument structs)
_GROUPS: dict = {}
_CAM_STRUCTS: dict = {}  # CameraParams values -> GsCamera (CameraParams.to_struct)


def _partial_groups(tile_size: int) -> int:
    g = _GROUPS.get(tile_size)
    if g is None:
        g = _GROUPS[tile_size] = int(N.load().gs_partial_groups(int(tile_size)))
    return g


# Memory budgets for tiles of many 8x8 cells (the default tile's four cells
# never batch, the performance path): the backward's [T, G] partials + flags
# per cell batch, and the forward's [cells, live_words] liveness bitmap
# (above it none is written and the backward replays every entry).
PARTIAL_BUDGET_BYTES = int(os.environ.get("GS_PARTIAL_BUDGET", str(2 << 30)))
LIVE_BUDGET_BYTES = int(os.environ.get("GS_LIVE_BUDGET", str(1 << 30)))
_ALWAYS_ONE_BATCH = 4  # cells


def cell_batch(cells: int, entries: int, slot_bytes: int = 41) -> int:
    """Cells per blend-backward batch for a frame of `entries` list entries:
    every cell at once unless the [entries, cells] partials (40 B) and flags
    (1 B) would exceed PARTIAL_BUDGET_BYTES; batches are summed in order by
    gs_gather_partials (deterministic, bounded memory).  slot_bytes: the
    scratch per (entry, cell) of another pass."""
    per = slot_bytes * max(int(entries), 1)
    if cells <= _ALWAYS_ONE_BATCH or cells * per <= PARTIAL_BUDGET_BYTES:
        return cells
    return max(1, min(cells, PARTIAL_BUDGET_BYTES // per))


def flag_groups(cells: int, cap: int, groups: int = 0) -> int:
    """Slot flags per entry of a tile workspace for `cap` entries (the
    flag_groups of gs_tile_workspace_bytes): the smallest count whose
    cap * flag_groups bytes hold [T, frame_groups(T)] for every T <= cap (the
    batch is chosen from the frame's own T, so that the summation order, and
    with it every gradient bit, depends on the frame only -- not on the
    capacity guess of the frame before).  groups: gs_partial_groups."""
    if 0 < groups < cells:
        return groups  # (combined cells: one batch)
    if cells <= _ALWAYS_ONE_BATCH:
        return cells
    # T * cell_batch(cells, T) <= max(min(cells * T, budget // 41), T) for every T
    return max(1, min(cells, -(-(PARTIAL_BUDGET_BYTES // 41) // max(int(cap), 1))))


def live_bitmap_bytes(lib, cells: int, entries: int, num_tiles: int) -> int:
    """Bytes of the forward's liveness bitmap, or 0 when it exceeds
    LIVE_BUDGET_BYTES (then none is written; ADVICE r04: at 1080p a tile of
    1920 px holds 57,600 cells, ~7 GB of bitmap for 1M Gaussians)."""
    nbytes = 8 * cells * int(lib.gs_blend_live_words(int(entries), int(num_tiles)))
    return nbytes if cells <= _ALWAYS_ONE_BATCH or nbytes <= LIVE_BUDGET_BYTES else 0


def _rows(t: torch.Tensor, cols: int) -> Tuple[torch.Tensor, int]:
    """(tensor, row stride in floats) without copying when rows are dense."""
    if t.dim() == 1 and cols == 1:
        return t, t.stride(0)
    if t.stride(-1) != 1 or t.shape[-1] != cols:
        t = t.contiguous()
    return t, t.stride(0)


_G_STRUCTS: dict = {}  # (pointers, strides, flags) -> GsGaussians (_gaussians_struct)


def _gaussians_struct(n, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit=False,
                      sh_rest=None, sh_degree=0) -> N.GsGaussians:
    """The ABI view of the Gaussians' tensors, cached by the addresses,
    strides and flags it holds (the same model renders with the same struct;
    callers copy it and never modify it)."""
    key = (n, xyz.data_ptr(), xyz.stride(0), None if cov3d is None else cov3d.data_ptr(),
           None if scaling is None else scaling.data_ptr(), None if rotation is None else rotation.data_ptr(),
           logits.data_ptr(), logits.stride(0), opacity.data_ptr(), opacity.stride(0), bool(opacity_is_logit),
           int(sh_degree), None if sh_rest is None or sh_degree <= 0 else (sh_rest.data_ptr(), sh_rest.stride(0)))
    g = _G_STRUCTS.get(key)
    if g is None:
        if len(_G_STRUCTS) >= 4096:
            _G_STRUCTS.clear()
        g = _G_STRUCTS[key] = _build_gaussians_struct(n, xyz, cov3d, scaling, rotation, logits, opacity,
                                                      opacity_is_logit, sh_rest, sh_degree)
    return g


def _build_gaussians_struct(n, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit=False,
                            sh_rest=None, sh_degree=0) -> N.GsGaussians:
    g = N.GsGaussians()
    g.n = n
    g.xyz, g.xyz_stride = N.ptr(xyz), xyz.stride(0)
    g.cov3d = N.ptr(cov3d)
    g.scaling, g.rotation = N.ptr(scaling), N.ptr(rotation)
    g.color_logits, g.color_stride = N.ptr(logits), logits.stride(0)
    g.opacity, g.opacity_stride = N.ptr(opacity), opacity.stride(0)
    g.opacity_is_logit = 1 if opacity_is_logit else 0
    if sh_degree > 0:
        g.sh_degree, g.sh_rest, g.sh_rest_stride = int(sh_degree), N.ptr(sh_rest), sh_rest.stride(0)
    return g


def _stream() -> int:
    return N.stream_ptr()


class StageTimer:
    """Optional per-stage HIP-event timing on the stream the kernels are
    launched on (torch's current stream).  Disabled unless a bench enables it;
    when disabled, mark() is a no-op."""
    enabled = False
    only = None  # optional set of stage names to record (the others cost nothing)
    events: list = []
    pairs: list = []  # (name, e0, e1): intervals the library records around one launch (pair())
    _pool: list = []  # created events, reused across resets (creating one costs more host time than recording)
    _used = 0
    _raw: list = []   # N.RawEvent pool for pair()
    _raw_used = 0

    @classmethod
    def _event(cls):
        if cls._used == len(cls._pool):
            cls._pool.append(torch.cuda.Event(enable_timing=True))
        e = cls._pool[cls._used]
        cls._used += 1
        return e

    @classmethod
    def mark(cls, name: str):
        if cls.enabled and (cls.only is None or name in cls.only):
            e = cls._event()
            e.record()
            cls.events.append((name, e))

    @classmethod
    def pair(cls, name: str):
        """(e0, e1) for a launch the library brackets itself (the frame
        backward's blend launch), or None when `name` is not timed."""
        if not (cls.enabled and (cls.only is None or name in cls.only)):
            return None
        while len(cls._raw) < cls._raw_used + 2:
            cls._raw.append(N.RawEvent())
        e0, e1 = cls._raw[cls._raw_used], cls._raw[cls._raw_used + 1]
        cls._raw_used += 2
        cls.pairs.append((name, e0, e1))
        return e0, e1

    @classmethod
    def reset(cls):
        cls.events, cls.pairs, cls._used, cls._raw_used = [], [], 0, 0

    @classmethod
    def durations_ms(cls):
        """{stage: [ms per occurrence]} -- stage = interval from its mark to
        the next, or a bracketed launch's own interval."""
        torch.cuda.synchronize()
        out = {}
        ev = cls.events
        for (name, e0), (_, e1) in zip(ev[:-1], ev[1:]):
            if name.startswith("~"):
                continue
            out.setdefault(name, []).append(e0.elapsed_time(e1))
        for name, e0, e1 in cls.pairs:
            out.setdefault(name, []).append(e0.elapsed_ms(e1))
        return out


def _check_inputs(xyz: torch.Tensor):
    if not xyz.is_cuda:
        raise RuntimeError("the MI355X renderer needs Gaussians on a HIP device (got %s); "
                           "there is no CPU path" % xyz.device)


class DensityStats:
    """The 3DGS density-control statistics of `n` Gaussians on `device`, three
    contiguous fp32 [n] tensors: grad_accum (sum over the views that saw a
    Gaussian of the NDC-unit norm of dL/d(its projected centre)), denom (how
    many views saw it) and max_radii (its largest screen radius in them).

    render(..., density_stats=stats) / rasterize(..., density_stats=stats)
    add that view to them at the end of its backward (gs_density_accumulate,
    on the backward's stream).  No backward, no statistics: a forward under
    torch.no_grad(), or one whose backward never runs, adds nothing; a second
    backward of the same frame (retain_graph) adds the view a second time.

    abs_grad=True: a fourth tensor, abs_accum (else None) -- the same sum with
    the absolute per-pixel gradients, sum_p |dL/dmu_x(p)| and sum_p |dL/dmu_y(p)|
    in place of the signed sums (AbsGS; gsplat's absgrad), which a large
    Gaussian's pixels cannot cancel.  Such a render takes the stage path (the
    same outputs and gradients, bit for bit), its blend backward is
    gs_blend_backward_abs and its last launch gs_density_accumulate_abs.  The
    absolute statistic covers the colour pass (and |the caller's cotangent on
    viewspace_points|): a feature image's or a distortion map's gradient adds
    to the signed sums only."""
    __slots__ = ("n", "grad_accum", "denom", "max_radii", "abs_accum")

    def __init__(self, n: int, device, abs_grad: bool = False):
        self.n = int(n)
        self.grad_accum, self.denom, self.max_radii = (
            torch.zeros((self.n,), dtype=torch.float32, device=device) for _ in range(3))
        self.abs_accum = torch.zeros((self.n,), dtype=torch.float32, device=device) if abs_grad else None

    @property
    def device(self) -> torch.device:
        return self.grad_accum.device

    def reset(self) -> None:
        for t in (self.grad_accum, self.denom, self.max_radii):
            t.zero_()
        if self.abs_accum is not None:
            self.abs_accum.zero_()

    def mean_grad(self) -> torch.Tensor:
        """grad_accum / denom, 0 where no view saw the Gaussian."""
        seen = self.denom > 0
        return torch.where(seen, self.grad_accum / self.denom.clamp_min(1.0), torch.zeros_like(self.grad_accum))

    def mean_abs_grad(self) -> torch.Tensor:
        """abs_accum / denom, 0 where no view saw the Gaussian (abs_grad=True only)."""
        if self.abs_accum is None:
            raise ValueError("these DensityStats keep no absolute gradients: DensityStats(n, device, abs_grad=True)")
        seen = self.denom > 0
        return torch.where(seen, self.abs_accum / self.denom.clamp_min(1.0), torch.zeros_like(self.abs_accum))


def _check_density_stats(stats, n: int, dev) -> None:
    if not isinstance(stats, DensityStats):
        raise TypeError(f"density_stats must be a DensityStats, got {type(stats).__name__}")
    if stats.n != n:
        raise ValueError(f"density_stats holds {stats.n} Gaussians, the render {n}")
    for name in ("grad_accum", "denom", "max_radii", "abs_accum"):
        t = getattr(stats, name)
        if t is None and name == "abs_accum":
            continue
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"density_stats.{name} must be a contiguous fp32 [{n}] tensor on {dev}, got "
                             f"{type(t).__name__}")
        if tuple(t.shape) != (n,) or t.dtype != torch.float32 or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"density_stats.{name} must be a contiguous fp32 [{n}] tensor on {dev}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")


def _accumulate_density(lib, cam: CameraParams, stats, n: int, vis, radii, grad_sums, g_means2d, s,
                        abs_sums=None) -> None:
    """One gs_density_accumulate: this view added to `stats` (the last launch
    of its backward).  grad_sums: the address of the [n, 10] sums the
    projection backward read, or None for a frame without a blend gradient.
    Statistics with abs_accum: one gs_density_accumulate_abs in its place;
    abs_sums: the [n, 2] sums of gs_gather_abs_partials, or None (no pixel
    cotangent: the view and its radii still count)."""
    if stats is None or n == 0:
        return
    a = N.GsDensityStatsArgs(n, int(cam.image_width), int(cam.image_height), N.ptr(vis), N.ptr(radii),
                             grad_sums, N.ptr(g_means2d), N.ptr(stats.grad_accum), N.ptr(stats.denom),
                             N.ptr(stats.max_radii))
    if stats.abs_accum is not None:
        aa = N.GsDensityAbsArgs(a, N.ptr(abs_sums) or None, N.ptr(stats.abs_accum))
        N.check(lib.gs_density_accumulate_abs(C.byref(aa), s), "gs_density_accumulate_abs")
        return
    N.check(lib.gs_density_accumulate(C.byref(a), s), "gs_density_accumulate")


class ContributionStats:
    """How much each of `n` Gaussians on `device` contributed to the frames
    rendered into it, with c_i(p) the blend's own weight of Gaussian i at
    pixel p: weight_sum (fp32, the sum of c over every pixel of every view),
    weight_max (fp32, the largest c anywhere: RadSplat's pruning score),
    pixels (int64, how many pixels it reached with c > 0) and views (int32,
    how many views saw it), each [n] and contiguous, starting at zero.

    render(..., contribution_stats=stats) / rasterize(..., contribution_stats=stats)
    add the view at the end of the forward; no backward is needed, and a
    render under torch.no_grad() counts."""
    __slots__ = ("n", "weight_sum", "weight_max", "pixels", "views")
    _DTYPES = (("weight_sum", torch.float32), ("weight_max", torch.float32), ("pixels", torch.int64),
               ("views", torch.int32))

    def __init__(self, n: int, device):
        self.n = int(n)
        for name, dtype in self._DTYPES:
            setattr(self, name, torch.zeros((self.n,), dtype=dtype, device=device))

    @property
    def device(self) -> torch.device:
        return self.weight_sum.device

    def reset(self) -> None:
        for name, _ in self._DTYPES:
            getattr(self, name).zero_()

    def mean_weight(self) -> torch.Tensor:
        """weight_sum / pixels, 0 where the Gaussian reached no pixel."""
        hit = self.pixels > 0
        return torch.where(hit, self.weight_sum / self.pixels.clamp_min(1).to(torch.float32),
                           torch.zeros_like(self.weight_sum))

    def all_reduce(self, dist) -> None:
        """Combine the ranks' statistics (each rank rendered other views):
        SUM, MAX, SUM, SUM.  dist: torch.distributed or a module like it."""
        if not self.n:
            return
        dist.all_reduce(self.weight_sum, op=dist.ReduceOp.SUM)
        dist.all_reduce(self.weight_max, op=dist.ReduceOp.MAX)
        dist.all_reduce(self.pixels, op=dist.ReduceOp.SUM)
        dist.all_reduce(self.views, op=dist.ReduceOp.SUM)


def _check_contribution_stats(stats, n: int, dev) -> None:
    if not isinstance(stats, ContributionStats):
        raise TypeError(f"contribution_stats must be a ContributionStats, got {type(stats).__name__}")
    if stats.n != n:
        raise ValueError(f"contribution_stats holds {stats.n} Gaussians, the render {n}")
    for name, dtype in ContributionStats._DTYPES:
        t = getattr(stats, name)
        if tuple(t.shape) != (n,) or t.dtype != dtype or not t.is_contiguous() or t.device != dev:
            raise ValueError(f"contribution_stats.{name} must be a contiguous {dtype} [{n}] tensor on {dev}, got "
                             f"{t.dtype} {tuple(t.shape)} on {t.device}")


class _ContributionPass:
    """What one render asked of the contribution pass (statistics to add the
    view to, or None; the dominant-Gaussian maps or not) and, after the
    forward, the maps."""
    __slots__ = ("stats", "dominant", "dominant_id", "dominant_weight")

    def __init__(self, stats, dominant: bool):
        self.stats, self.dominant, self.dominant_id, self.dominant_weight = stats, bool(dominant), None, None


def contribution_cell_batch(cells: int, entries: int) -> int:
    """cell_batch's rule for the contribution pass's scratch: 16 B of partial
    and 1 B of flag per (entry, cell)."""
    return cell_batch(cells, entries, 17)


def _contribution_pass(cam: CameraParams, fr: "_Frame", n: int, cp: _ContributionPass, dev) -> None:
    """The contribution pass over a stage-path frame, at the end of its
    forward: per cell batch one gs_blend_contributions into scratch partials
    and flags of its own (the backward's are not touched) and, with
    statistics, one gs_contrib_accumulate."""
    H, W = int(cam.image_height), int(cam.image_width)
    if cp.dominant:
        cp.dominant_id = torch.empty((H, W), dtype=torch.int32, device=dev)
        cp.dominant_weight = torch.empty((H, W), dtype=torch.float32, device=dev)
    if fr.M == 0 or fr.T == 0:
        if cp.dominant:
            cp.dominant_id.fill_(-1)
            cp.dominant_weight.zero_()
        return
    lib = N.load()
    s = _stream()
    T, Q = fr.T, cam.cells
    G = contribution_cell_batch(Q, T)
    partials = torch.empty((T * G, N.GS_CONTRIB_STRIDE), dtype=torch.float32, device=dev)
    flags = torch.empty((T * G,), dtype=torch.uint8, device=dev)
    ca = N.GsContribArgs(replay_frame(cam, fr, n), N.ptr(partials), N.ptr(flags), 0, 0, N.ptr(cp.dominant_id),
                         N.ptr(cp.dominant_weight))
    st = cp.stats
    if st is not None:
        ga = N.GsContribGatherArgs(n, N.ptr(fr.vis), N.ptr(fr.rects), N.ptr(fr.pair_offset), N.ptr(partials),
                                   N.ptr(flags), G, 1, N.ptr(st.weight_sum), N.ptr(st.weight_max), N.ptr(st.pixels),
                                   N.ptr(st.views))
    for b, c0 in enumerate(range(0, Q, G)):
        ca.cell_begin, ca.cell_count = c0, min(G, Q - c0)
        flags.zero_()
        StageTimer.mark("contrib_blend")
        N.check(lib.gs_blend_contributions(C.byref(ca), s), "gs_blend_contributions")
        if st is not None:
            ga.partial_groups, ga.first_batch = ca.cell_count, (0 if b else 1)
            StageTimer.mark("contrib_gather")
            N.check(lib.gs_contrib_accumulate(C.byref(ga), s), "gs_contrib_accumulate")
    StageTimer.mark("~end_contrib")


def check_distortion_near_far(near_far) -> Tuple[float, float]:
    """(near, far) of the distortion's depth map as the kernels take them:
    (0, 0), linear depth, for None; else two finite numbers with
    0 < near < far (the inverse map) -- anything else is a ValueError."""
    if near_far is None:
        return 0.0, 0.0
    try:
        near, far = (float(v) for v in near_far)
    except (TypeError, ValueError):
        raise ValueError(f"distortion_near_far must be None or (near, far), got {near_far!r}") from None
    if not (math.isfinite(near) and math.isfinite(far) and 0.0 < near < far):
        raise ValueError(f"distortion_near_far needs finite 0 < near < far, got {near_far!r}")
    return near, far


class _DistortionPass:
    """What one render asked of the distortion pass (the depth map's planes)
    and, after the forward, its non-differentiable maps: median_depth,
    median_id, and moments [2, H, W] = (A_n, S_n), the backward's state."""
    __slots__ = ("near", "far", "moments", "median_depth", "median_id")

    def __init__(self, near_far=None):
        self.near, self.far = check_distortion_near_far(near_far)
        self.moments = self.median_depth = self.median_id = None


class _DistortionGrad:
    """One backward's view of a frame's distortion pass: the pass, the
    forward's distortion map and its cotangent."""
    __slots__ = ("dp", "out", "g_out")

    def __init__(self, dp, out, g_out):
        self.dp, self.out, self.g_out = dp, out, g_out


def _live_words(fr) -> int:
    return 0 if fr.live_bits is None else fr.live_bits.shape[1]


def replay_frame(cam: CameraParams, fr, n: int) -> N.GsReplayFrame:
    """gs_replay_frame of a stage-path frame `fr` of n Gaussians: the colour
    forward's saved state, the first member of every replay's arguments."""
    return N.GsReplayFrame(cam.to_struct(), cam.tiles_x, cam.tiles_y, N.ptr(fr.ranges), N.ptr(fr.sorted_gauss),
                           N.ptr(fr.records), N.ptr(fr.cell_neval), N.ptr(fr.live_bits), _live_words(fr), fr.T, n)


def _fp32_contiguous(t: torch.Tensor) -> torch.Tensor:
    """A cotangent as the kernels read it."""
    return t if t.dtype == torch.float32 and t.is_contiguous() else t.to(torch.float32).contiguous()


def _distortion_forward(cam: CameraParams, fr: "_Frame", n: int, dp: _DistortionPass, dev) -> torch.Tensor:
    """The distortion map [H, W] of a stage-path frame, and dp's maps: one
    gs_blend_distortion_forward over the state the colour forward left in
    `fr` (zeros / -1 when nothing was drawn)."""
    H, W, f32 = int(cam.image_height), int(cam.image_width), torch.float32
    fr.distortion = dp  # (where the tests read the moments)
    if fr.M == 0 or fr.T == 0:
        dp.moments = torch.zeros((2, H, W), dtype=f32, device=dev)
        dp.median_depth = torch.zeros((H, W), dtype=f32, device=dev)
        dp.median_id = torch.full((H, W), -1, dtype=torch.int32, device=dev)
        return torch.zeros((H, W), dtype=f32, device=dev)
    out = torch.empty((H, W), dtype=f32, device=dev)
    dp.moments = torch.empty((2, H, W), dtype=f32, device=dev)
    dp.median_depth = torch.empty((H, W), dtype=f32, device=dev)
    dp.median_id = torch.empty((H, W), dtype=torch.int32, device=dev)
    fa = N.GsDistortionFwdArgs(replay_frame(cam, fr, n), dp.near, dp.far, N.ptr(out), N.ptr(dp.moments),
                               N.ptr(dp.median_depth), N.ptr(dp.median_id))
    StageTimer.mark("distortion_fwd")
    N.check(N.load().gs_blend_distortion_forward(C.byref(fa), _stream()), "gs_blend_distortion_forward")
    StageTimer.mark("~end_distortion_fwd")
    return out


class _GradSums:
    """One backward's per-Gaussian sums over a stage-path frame, [n,
    GS_PAIR_GRAD_FLOATS] (the frame workspace's grad_sums, as
    gs_render_backward uses it), and what every pass needs
    to add to them: the frame's gather arguments, whether the sums hold
    anything yet (the next gather's `accumulate`), and the colour pass's
    partial buffer -- with its flags while its one batch is not yet gathered."""
    __slots__ = ("fr", "n", "dev", "_sums", "have", "partials", "flags")

    def __init__(self, fr: "_Frame", n: int, dev):
        self.fr, self.n, self.dev = fr, n, dev
        self._sums, self.have, self.partials, self.flags = None, False, None, None

    @property
    def sums(self) -> torch.Tensor:
        if self._sums is None:
            self._sums = self.fr.grad_sums
        return self._sums

    def accumulate(self) -> int:
        """The `accumulate` of the next gather into the sums: 0 for the first, which stores."""
        acc, self.have = (1 if self.have else 0), True
        return acc

    def gather_args(self, pair_grads, slot_live) -> "N.GsProjectBwdArgs":
        """gs_gather_partials' arguments for the frame's slots of (pair_grads, slot_live)."""
        ga, fr = N.GsProjectBwdArgs(), self.fr
        ga.g.n = self.n
        ga.vis, ga.rects, ga.pair_offset = N.ptr(fr.vis), N.ptr(fr.rects), N.ptr(fr.pair_offset)
        ga.pair_grads, ga.slot_live, ga.grad_sums = N.ptr(pair_grads), N.ptr(slot_live), N.ptr(self.sums)
        return ga

    def gather(self, lib, ga: "N.GsProjectBwdArgs", groups: int, s) -> None:
        """One gs_gather_partials of ga's partials, `groups` per slot, into the sums."""
        ga.partial_groups = groups
        N.check(lib.gs_gather_partials(C.byref(ga), self.accumulate(), s), "gs_gather_partials")

    def scratch(self, lib, s):
        """(partials [T G, GS_PARTIAL_STRIDE], flags [T G]) for a pass after the
        colour pass, G = the frame's cells per batch: the colour pass's partials
        are gathered first if they still wait, and their buffer is reused when
        it is large enough.  The flags are the pass's own, cleared by it before
        every launch."""
        rows = self.fr.T * self.fr.groups
        if self.flags is not None:
            self.gather(lib, self.gather_args(self.partials, self.flags), self.fr.groups, s)
            self.flags = None
        if self.partials is None or self.partials.shape[0] < rows:
            self.partials = torch.empty((rows, N.GS_PARTIAL_STRIDE), dtype=torch.float32, device=self.dev)
        return self.partials, torch.empty((rows,), dtype=torch.uint8, device=self.dev)

    def for_projection(self):
        """(pair_grads, slot_live, grad_sums) of the projection backward: the
        colour pass's partials and flags with a buffer to sum them into, or the
        sums gathered so far, or nothing (no blend gradient)."""
        if self.flags is not None:
            return self.partials, self.flags, self.sums
        return None, None, (self._sums if self.have else None)


def _distortion_backward(lib, cam: CameraParams, fr: "_Frame", dist: _DistortionGrad, sums: _GradSums, s) -> None:
    """The distortion's backward over a stage-path frame: per cell batch (the
    frame's own plan: fr.groups cells at a time) one
    gs_blend_distortion_backward and one gs_gather_partials that adds its
    partials to `sums`."""
    G, Q = fr.groups, cam.cells
    pair_grads, flags = sums.scratch(lib, s)
    dp = dist.dp
    g_out = _fp32_contiguous(dist.g_out)
    ba = N.GsDistortionBwdArgs(replay_frame(cam, fr, sums.n), dp.near, dp.far, N.ptr(dist.out), N.ptr(dp.moments),
                               N.ptr(g_out), N.ptr(pair_grads), N.ptr(flags), 0, 0)
    ga = sums.gather_args(pair_grads, flags)
    StageTimer.mark("distortion_bwd")
    for c0 in range(0, Q, G):
        ba.cell_begin, ba.cell_count = c0, min(G, Q - c0)
        flags.zero_()
        N.check(lib.gs_blend_distortion_backward(C.byref(ba), s), "gs_blend_distortion_backward")
        sums.gather(lib, ga, ba.cell_count, s)
    StageTimer.mark("~end_distortion_bwd")


_FRAME_LAYOUTS: dict = {}  # (n, W, H, tile) -> N.FrameOffsets (.total: gs_frame_workspace_bytes)


def _frame_layout(n: int, W: int, H: int, tile: int) -> "N.FrameOffsets":
    key = (n, W, H, tile)
    fo = _FRAME_LAYOUTS.get(key)
    if fo is None:
        fo = _FRAME_LAYOUTS[key] = N.frame_offsets(n, W, H, tile)
    return fo


class _Frame:
    """One forward's state for its backward and the replays, whichever host
    path made it (calls: gs_render_forward did): the camera, the frame
    workspace (per Gaussian and per pixel) and the tile workspace (per list
    entry) as the library lays them out (fb: their gs_frame_buffers), and what
    the forward learned -- M, T, which ping-pong halves hold the sorted ids
    (depth_alt, tile_alt), and groups, the backward's partials per entry and
    batch.  flags_zeroed: the slot flags still hold the forward's zeros (a
    forward with need_grad, until the first backward's colour pass).  The
    buffers are views made on demand from the named offsets (fo, to)."""
    __slots__ = ("cam", "fb", "fo", "frame_ws", "tile_ws", "n", "M", "T", "groups", "depth_alt", "tile_alt", "vis",
                 "flags_zeroed", "distortion", "calls", "tiles", "cells", "_to")

    def __init__(self, cam: CameraParams, n: int, vis, calls: bool):
        """A frame of n Gaussians with its frame workspace; the forward fills in the rest."""
        self.cam, self.n, self.vis, self.calls = cam.to_struct(), n, vis, calls
        self.tiles, self.cells, self.groups = cam.tiles_x * cam.tiles_y, cam.cells, cam.groups
        self.fo = _frame_layout(n, int(cam.image_width), int(cam.image_height), cam.tile_size)
        self.frame_ws = torch.empty((self.fo.total,), dtype=torch.uint8, device=vis.device)
        self.fb = self.tile_ws = self.distortion = self._to = None
        self.M = self.T = self.depth_alt = self.tile_alt = 0
        self.flags_zeroed = False

    @property
    def to(self) -> "N.TileOffsets":
        """The layout of tile_ws, the workspace fb names."""
        if self._to is None:
            fb = self.fb
            self._to = N.tile_offsets(fb.capacity, self.tiles, fb.live_cells, fb.flag_groups)
        return self._to

    def _f(self, off, nbytes, dtype, shape):
        return self.frame_ws[off:off + nbytes].view(dtype).view(shape)

    def _t(self, off, nbytes, dtype, shape):
        return self.tile_ws[off:off + nbytes].view(dtype).view(shape)

    records = property(lambda s: s._f(s.fo.records, 4 * N.GS_RECORD_FLOATS * s.n, torch.float32,
                                      (s.n, N.GS_RECORD_FLOATS)))
    rects = property(lambda s: s._f(s.fo.rects, 8 * s.n, torch.int32, (s.n, 2)))
    order = property(lambda s: s._f(s.fo.vals, 8 * s.n, torch.int32, (2, s.n))[s.depth_alt])
    counters = property(lambda s: s._f(s.fo.counters, 4 * N.GS_NUM_COUNTERS, torch.int32, (N.GS_NUM_COUNTERS,)))
    pair_offset = property(lambda s: s._f(s.fo.pair_offset, 4 * s.n, torch.int32, (s.n,)))
    ranges = property(lambda s: s._f(s.fo.ranges, 8 * s.tiles, torch.int32, (s.tiles, 2)))
    pix_flags = property(lambda s: s._f(s.fo.pix_flags, s.cam.image_width * s.cam.image_height, torch.uint8, (-1,)))
    cell_neval = property(lambda s: s._f(s.fo.cell_neval, 4 * s.tiles * s.cells, torch.int32, (s.tiles, s.cells)))
    grad_sums = property(lambda s: s._f(s.fo.grad_sums, 4 * N.GS_PAIR_GRAD_FLOATS * s.n, torch.float32,
                                        (s.n, N.GS_PAIR_GRAD_FLOATS)))
    sorted_gauss = property(lambda s: s._t(s.to.tv1 if s.tile_alt else s.to.tv0, 4 * s.T, torch.int32, (s.T,)))
    live_bits = property(lambda s: s._t(s.to.live, 8 * s.cells * s.to.live_words, torch.int64,
                                        (s.cells, s.to.live_words)) if s.fb.live_cells else None)
    slot_live = property(lambda s: s._t(s.to.flags, s.groups * s.T, torch.uint8, (s.groups * s.T,)))


class _FastFrame(_Frame):
    """A _Frame with `calls` set, under the name the call path's frame had
    before, plus fa, the arguments gs_render_forward filled in (the depth-bit
    range it reported: tests/device_frame_util.host_frame compares it with the
    device-resident frame's).  Tests written against the two former classes
    tell a call-path frame by isinstance(fr, _FastFrame) and read fr.fa; they
    keep passing.  The state and the views are _Frame's, and nothing in the
    package tells the two apart."""
    __slots__ = ("fa",)


_T_SEEN: dict = {}  # device -> tile entries T of its last frame (capacity guess)
# per host thread: device -> pinned int32[4] for the (M, T, depth-bits range)
# read-back (renders from several threads each read their own counters; the
# two per-device guesses above are only guesses, a stale one is corrected)
_HOST_COUNTERS = threading.local()


class _HostCounters:
    """Pinned int32[8] gs_bin_count writes (M, T, depth-bits min / max) and
    then a sequence word into, through its device address: the host polls the
    word -- no copy and no event in the stream (an event record between the
    count and the emission cost a ~6 us gap on the GPU).  Without a device
    address (dptr None) the counters are copied and an event is waited for."""
    __slots__ = ("t", "np", "dptr", "seq")

    def __init__(self):
        self.t = torch.empty((8,), dtype=torch.int32, pin_memory=True)
        self.np = self.t.numpy()
        self.dptr = N.host_device_pointer(self.t)
        self.seq = 0

    def next_seq(self) -> int:
        """This frame's sequence word (1 .. 2^31 - 1, never the cleared 0)."""
        self.seq = self.seq % 0x7FFFFFFF + 1
        return self.seq

    def arm(self, ba) -> None:
        if self.dptr is None:
            return
        self.np[4] = 0  # (the previous frame's word; the GPU writes this frame's after its counters)
        ba.host_counters, ba.host_seq = self.dptr, self.next_seq()

    def wait(self, dev, ready) -> Tuple[int, int, int, int]:
        if self.dptr is None:
            ready.synchronize()
        else:
            hv, seq, i = self.np, self.seq, 0
            deadline = time.perf_counter() + 10.0
            while hv[4] != seq:
                i += 1
                if (i & 255) == 0:
                    if time.perf_counter() > deadline:  # (never in a healthy run)
                        torch.cuda.synchronize(dev)
                        if hv[4] != seq:
                            raise RuntimeError("gs_bin_count: the frame's counters never reached the host")
                        break
                    time.sleep(0)  # other host threads get the interpreter
        v = self.np[:4].tolist()
        return int(v[0]), int(v[1]), int(v[2]) & 0xFFFFFFFF, int(v[3]) & 0xFFFFFFFF
_FUSE_FLAGS = os.environ.get("GS_FUSE_SLOT_FLAGS", "1") != "0"  # slot flags zeroed by gs_tile_ranges
# Depth-key windows (per process and device; these are guesses, a stale one
# only costs a re-render, so host threads may race on them): the window
# covers the union of the last _WINDOW_FRAMES frames' visible depth ranges, so
# views that alternate (a trainer's shuffled cameras) keep fitting it.  A
# frame whose depths leave the window (a miss) is rendered again with 32-bit
# keys; a second miss within _MISS_SPAN frames turns windows off for
# _WINDOW_OFF_FRAMES frames (a miss costs a whole re-render, a window saves
# ~20 us of sorting).
_DEPTH_HIST: dict = {}  # device -> [(zmin_bits, zmax_bits)] of its last frames
_WINDOW_FRAMES = 8
_MISS_SPAN = 32
_WINDOW_OFF_FRAMES = 256
_WINDOW_STATE: dict = {}  # device -> {"frame", "misses", "last_miss", "off_until"}
# Windowed depth keys of 9..31 bits are sorted by gs_depth_sort_msd (one MSD pass + a sort per
# bucket in LDS) unless GS_DEPTH_MSD=0.  A bucket over its LDS capacity (clumped depths) poisons
# the frame's depth max (0xFFFFFFFF): the frame is sorted again with the LSD passes, and the LSD
# path is kept for the next _MSD_BACKOFF_FRAMES frames on that device.
_DEPTH_MSD = os.environ.get("GS_DEPTH_MSD", "1") != "0"
_MSD_BACKOFF: dict = {}  # device -> frames left on the LSD path after an overflow
_MSD_BACKOFF_FRAMES = 64
_POISON = 0xFFFFFFFF


def depth_window(zmin_bits: int, zmax_bits: int):
    """(key_base, key_bits) of a window around the visible fp32 depth bits
    [zmin_bits, zmax_bits], widened by 1/8 of the range on both sides for the
    next frame's drift; None when the range needs all 32 bits.  Windows of 25-31
    bits save no LSD pass, but they keep the depth sort on gs_depth_sort_msd
    (raw fp32 bits would put every key into one MSD bucket)."""
    if zmin_bits > zmax_bits:
        return None
    span = zmax_bits - zmin_bits
    lo = max(0, zmin_bits - span // 8 - 1)
    hi = zmax_bits + span // 8 + 1
    bits = max(1, (hi - lo + 1).bit_length())  # keys 0 .. hi - lo < 2^bits - 1 (the culled sentinel)
    if bits >= 9 and hi - lo >= _msd_limit(bits):
        bits += 1  # the MSD depth sort's top bucket is the sentinel's alone
    return (lo, bits) if bits < 32 else None


def _msd_limit(bits: int) -> int:
    """Visible keys of a `bits`-bit window stay below this: 2^bits - 1 (the
    culled sentinel) and, from 9 bits on, 255 << (bits - 8), so that the top
    digit of gs_depth_sort_msd's MSD pass holds the sentinel only."""
    return min((1 << bits) - 1, 255 << (bits - 8)) if bits >= 9 else (1 << bits) - 1


def _window_state(dev) -> dict:
    st = _WINDOW_STATE.get(dev)
    if st is None:
        st = _WINDOW_STATE[dev] = {"frame": 0, "misses": 0, "last_miss": None, "off_until": 0}
    return st


def _window_for(dev):
    """The depth-key window of this device's next frame (None: 32-bit keys)."""
    st = _window_state(dev)
    hist = _DEPTH_HIST.get(dev)
    if not hist or st["frame"] < st["off_until"]:
        return None
    return depth_window(min(h[0] for h in hist), max(h[1] for h in hist))


def _record_depths(dev, zmin_bits: int, zmax_bits: int) -> None:
    """A finished frame's visible depth-bit range (none visible: nothing)."""
    st = _window_state(dev)
    st["frame"] += 1
    if zmin_bits > zmax_bits:
        return
    hist = _DEPTH_HIST.setdefault(dev, [])
    hist.append((zmin_bits, zmax_bits))
    del hist[:-_WINDOW_FRAMES]


def _note_window_miss(dev) -> None:
    st = _window_state(dev)
    st["misses"] += 1
    if st["last_miss"] is not None and st["frame"] - st["last_miss"] <= _MISS_SPAN:
        st["off_until"] = st["frame"] + _WINDOW_OFF_FRAMES
    st["last_miss"] = st["frame"]


def depth_window_stats(dev=None) -> dict:
    """Frames rendered and window misses (re-renders) per device: a
    measurement of the depth-key window's hit rate."""
    if dev is not None:
        return dict(_window_state(torch.device(dev)))
    return {str(d): dict(v) for d, v in _WINDOW_STATE.items()}


def window_holds(window, zmin_bits: int, zmax_bits: int) -> bool:
    """Did every visible key of this frame fit the window it was sorted with?"""
    if window is None or zmin_bits > zmax_bits:
        return True
    base, bits = window
    return zmin_bits >= base and zmax_bits - base < _msd_limit(bits)


# The per-frame decisions every host path takes from the state above (the
# stage path, the frame entry points, graph_step.GraphedStep's capture).

def _capacity_guess(dev) -> int:
    """Tile entries to make room for before this device's next T is known:
    its last frame's T and a quarter, plus 4096; 0 when no frame was seen."""
    seen = _T_SEEN.get(dev, 0)
    return seen + seen // 4 + 4096 if seen else 0


def _depth_keys(dev, depth_window_ok: bool, consume: bool = True, window="auto"):
    """(window, key_base, key_bits, msd) of this device's next depth sort: the
    window of _window_for (none without depth_window_ok, or the caller's own),
    32-bit keys without one, and whether gs_depth_sort_msd sorts them.  The MSD
    backoff counts only frames that would have taken the MSD sort (it is per
    process and device, not per host thread); a capture (consume=False) looks
    at it without spending a frame of it."""
    if window == "auto":
        window = _window_for(dev) if depth_window_ok else None
    key_base, key_bits = window if window is not None else (0, 32)
    msd = _DEPTH_MSD and window is not None and 9 <= key_bits <= 31
    backoff = _MSD_BACKOFF.get(dev, 0)
    if msd and backoff and consume:
        _MSD_BACKOFF[dev] = backoff - 1
    return window, key_base, key_bits, bool(msd and not backoff)


def _frame_missed(dev, depth_max_bits: int, T: int) -> None:
    """A frame to render again with 32-bit keys: a visible depth outside the
    window (the sort's keys were clipped), or an MSD bucket over capacity (the
    depth max poisoned)."""
    if depth_max_bits == _POISON:
        _MSD_BACKOFF[dev] = _MSD_BACKOFF_FRAMES
    else:
        _note_window_miss(dev)
    _T_SEEN[dev] = T


def _frame_done(dev, T: int, zmin_bits: int, zmax_bits: int) -> None:
    """A finished frame's T and visible depth range: the next frame's guesses."""
    _T_SEEN[dev] = T
    _record_depths(dev, zmin_bits, zmax_bits)


# Frames at the default tile run through the library's frame entry points
# (gs_render_forward / gs_render_backward: one call per direction over two
# workspaces, ABI 18) unless GS_FRAME_CALLS=0; other tile sizes, and hosts
# whose pinned counters have no device address, take the stage-by-stage path
# below.  The two paths launch the same kernels on the same data: their
# outputs and gradients are bit-identical (test_frame_entry_points_match).
_FRAME_CALLS = os.environ.get("GS_FRAME_CALLS", "1") != "0"
# gs_render_forward's patience with the counter poll before it synchronises the
# stream and looks once more (0: the library's 10 s; tests shorten it)
_POLL_TIMEOUT_MS = int(os.environ.get("GS_POLL_TIMEOUT_MS", "0"))


def _host_counters(dev) -> "_HostCounters":
    per_thread = getattr(_HOST_COUNTERS, "bufs", None)
    if per_thread is None:
        per_thread = _HOST_COUNTERS.bufs = {}
    hc = per_thread.get(dev)
    if hc is None:
        hc = per_thread[dev] = _HostCounters()
    return hc


def _gaussian_outputs(n: int, dev):
    """A forward's per-Gaussian outputs: means2d, conics, radii, vis."""
    f32 = torch.float32
    return (torch.empty((n, 2), dtype=f32, device=dev), torch.empty((n, 2, 2), dtype=f32, device=dev),
            torch.empty((n,), dtype=f32, device=dev), torch.empty((n,), dtype=torch.bool, device=dev))


def _pixel_outputs(H: int, W: int, dev):
    """A forward's per-pixel outputs: image, alpha, depth."""
    f32 = torch.float32
    return (torch.empty((3, H, W), dtype=f32, device=dev), torch.empty((1, H, W), dtype=f32, device=dev),
            torch.empty((1, H, W), dtype=f32, device=dev))


def _empty_frame_outputs(cam: CameraParams, dev):
    """image, alpha, depth of a frame that draws nothing (M == 0).
    renderer.py:74-83: bg once (not doubled, not clamped), zero alpha/depth"""
    H, W, f32 = int(cam.image_height), int(cam.image_width), torch.float32
    image = torch.tensor(cam.bg, dtype=f32, device=dev).view(3, 1, 1).repeat(1, H, W)
    return image, torch.zeros((1, H, W), dtype=f32, device=dev), torch.zeros((1, H, W), dtype=f32, device=dev)


def _bind_frame_args(fa: "N.GsRenderFwdArgs", cam: CameraParams, gst, gaussian_outs, pixel_outs, frame_ws) -> None:
    """The fields of gs_render_forward's arguments every caller fills alike:
    camera, Gaussians, the seven outputs and the frame workspace."""
    fa.cam, fa.g = cam.to_struct(), gst
    if cam.screen_filter:  # (fa is zeroed: no filter)
        fa.filter = cam.filter_struct()
    fa.means2d, fa.conics, fa.radii, fa.vis = (t.data_ptr() for t in gaussian_outs)
    fa.image, fa.alpha, fa.depth = (t.data_ptr() for t in pixel_outs)
    fb = fa.fb
    fb.frame_ws, fb.frame_ws_bytes = frame_ws.data_ptr(), frame_ws.numel()
    fb.live_cells, fb.flag_groups = cam.cells, cam.groups


def _bind_tile_ws(fa: "N.GsRenderFwdArgs", tile_ws, cap: int) -> None:
    """A tile workspace of gs_tile_workspace_bytes(cap, ...) bytes for `cap` entries."""
    fb = fa.fb
    fb.tile_ws, fb.tile_ws_bytes, fb.capacity = tile_ws.data_ptr(), tile_ws.numel(), cap


def _forward_frame(cam: CameraParams, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit, sh_rest,
                   sh_degree, pair_counts, depth_window_ok, need_grad, hc, pix_neval):
    """forward_pipeline through gs_render_forward (the default tile)."""
    lib = N.load()
    dev = xyz.device
    n = int(xyz.shape[0])
    H, W = int(cam.image_height), int(cam.image_width)
    s = _stream()
    fa = N.GsRenderFwdArgs()
    means2d, conics, radii, vis = gaussian_outs = _gaussian_outputs(n, dev)
    image, alpha, depth = pixel_outs = _pixel_outputs(H, W, dev)
    fr = _FastFrame(cam, n, vis, calls=True)
    fr.fa = fa
    _bind_frame_args(fa, cam, _gaussians_struct(n, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit,
                                                sh_rest, sh_degree), gaussian_outs, pixel_outs, fr.frame_ws)

    def tile_workspace(cap):
        tws = int(lib.gs_tile_workspace_bytes(cap, fr.tiles, cam.cells, cam.groups))
        ws = torch.empty((tws,), dtype=torch.uint8, device=dev)
        _bind_tile_ws(fa, ws, cap)
        return ws
    cap = _capacity_guess(dev)
    tile_ws = tile_workspace(cap) if cap else None
    _, fa.key_base, fa.key_bits, msd = _depth_keys(dev, depth_window_ok)
    fa.depth_sort_msd = 1 if msd else 0
    fa.zero_slot_flags = 1 if need_grad else 0
    fa.host_counters_dev, fa.host_counters_host, fa.host_seq = hc.dptr, hc.t.data_ptr(), hc.next_seq()
    fa.pair_counts, fa.pix_neval = N.ptr(pair_counts), N.ptr(pix_neval)
    fa.poll_timeout_ms = _POLL_TIMEOUT_MS
    st = lib.gs_render_forward(C.byref(fa), s)
    if st == N.GS_RETRY_FULL_KEYS:
        _frame_missed(dev, fa.depth_max_bits, fa.T)
        return forward_pipeline(cam, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit,
                                sh_rest, sh_degree, pair_counts, depth_window_ok=False, need_grad=need_grad,
                                pix_neval=pix_neval)
    if st == N.GS_NEED_CAPACITY:
        tile_ws = tile_workspace(fa.T)
        fa.resume = 1
        st = lib.gs_render_forward(C.byref(fa), s)
    N.check(st, "gs_render_forward")
    M, T = int(fa.M), int(fa.T)
    if n > 0:
        _frame_done(dev, T, int(fa.depth_min_bits), int(fa.depth_max_bits))
    fr.fb, fr.tile_ws, fr.M, fr.T, fr.depth_alt, fr.tile_alt = fa.fb, tile_ws, M, T, fa.depth_alt, fa.tile_alt
    fr.flags_zeroed = bool(need_grad)
    if M == 0:
        image, alpha, depth = _empty_frame_outputs(cam, dev)
    return image, alpha, depth, means2d, conics, radii, vis, fr


def forward_pipeline(cam: CameraParams, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit=False,
                     sh_rest=None, sh_degree=0, pair_counts=None, depth_window_ok=True, need_grad=False,
                     pix_neval=None, stage_path=False):
    """stage_path: take the stage-by-stage path below at the default tile too
    (the feature pass reads the frame's buffers as tensors; the two paths'
    outputs and gradients are bit-identical).
    pair_counts / pix_neval: optional int32 [H*W] the blend fills with each
    pixel's contributing pairs / evaluated entries (measurement counters,
    SURVEY 8d, and the oracle's decision-forced replay; not in render()).

    The depth sort runs over a window of the depth keys' bits chosen from the
    previous frame's visible depth range on this device (one radix pass less
    per 8 bits, gs_project_args.key_base); this frame's range, read back with
    (M, T), says whether the window held -- if not, the frame is rendered
    again with full 32-bit keys (depth_window_ok=False)."""
    if _FRAME_CALLS and cam.tile_size == N.GS_DEFAULT_TILE and not stage_path:
        hc = _host_counters(xyz.device)
        if hc.dptr is not None:
            return _forward_frame(cam, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit, sh_rest,
                                  sh_degree, pair_counts, depth_window_ok, need_grad, hc, pix_neval)
    lib = N.load()
    dev = xyz.device
    n = int(xyz.shape[0])
    H, W = int(cam.image_height), int(cam.image_width)
    s = _stream()
    cs = cam.to_struct()
    gst = _gaussians_struct(n, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit, sh_rest, sh_degree)
    num_tiles = cam.tiles_x * cam.tiles_y
    bits = max(1, int(math.ceil(math.log2(num_tiles))) if num_tiles > 1 else 1)  # (of the tile sort's keys)

    # the frame workspace holds everything whose size does not depend on T, so
    # it is allocated before the one host sync: the GPU waits only for the
    # read-back and launches
    means2d, conics, radii, vis = _gaussian_outputs(n, dev)
    fr = _Frame(cam, n, vis, calls=False)
    fo, fw = fr.fo, fr.frame_ws.data_ptr()
    fb = fr.fb = N.GsFrameBuffers(fw, fo.total)
    keys, vals, key_minmax = fw + fo.keys, fw + fo.vals, fw + fo.key_minmax  # (keys, vals: [2, n] ping-pong)
    window, key_base, key_bits, msd = _depth_keys(dev, depth_window_ok)

    StageTimer.mark("project_fwd")
    pa = N.GsProjectArgs(cs, gst, N.ptr(means2d), N.ptr(conics), N.ptr(radii), N.ptr(vis), fw + fo.records,
                         fw + fo.rects, keys, key_base, key_bits, key_minmax, cam.filter_struct())
    N.check(lib.gs_project_forward(C.byref(pa), s), "gs_project_forward")

    def tile_workspace(cap: int):
        """(a tile workspace for `cap` entries, bound to fb; its layout; its tile sort's workspace bytes:
        what the capacity needs, >= what any T below it does) -- everything the launches after the sync
        need but T, laid out while the GPU counts and emits"""
        fb.live_cells = cam.cells if live_bitmap_bytes(lib, cam.cells, cap, num_tiles) else 0
        fb.flag_groups, fb.capacity = flag_groups(cam.cells, cap, cam.groups), cap
        to = N.tile_offsets(cap, num_tiles, fb.live_cells, fb.flag_groups)
        ws = torch.empty((to.total,), dtype=torch.uint8, device=dev)
        fb.tile_ws, fb.tile_ws_bytes = ws.data_ptr(), to.total
        ba.tile_keys, ba.pair_gauss, ba.capacity = fb.tile_ws + to.tk0, fb.tile_ws + to.tv0, cap
        return ws, to, lib.gs_radix_sort_workspace_bytes(cap)
    if n > 0:
        StageTimer.mark("depth_sort")
        alt = C.c_int32(0)
        ws_bytes = lib.gs_radix_sort_workspace_bytes(n)
        if msd:
            N.check(lib.gs_depth_sort_msd(keys, vals, keys + 4 * n, vals + 4 * n, n, key_bits, fw + fo.sort_ws,
                                          ws_bytes, key_minmax + 4, C.byref(alt), s), "depth sort (msd)")
        else:
            N.check(lib.gs_radix_sort_pairs(keys, vals, keys + 4 * n, vals + 4 * n, n, 0, key_bits, 1,
                                            fw + fo.sort_ws, ws_bytes, C.byref(alt), s), "depth sort")
        fr.depth_alt = alt.value
        ba = N.GsBinArgs(n, cam.tiles_x, cam.tiles_y, vals + 4 * n * alt.value, fw + fo.rects, N.ptr(vis),
                         fw + fo.counters, key_minmax, fw + fo.bin_ws, lib.gs_bin_workspace_bytes(n), 0, 0,
                         fw + fo.pair_offset, fw + fo.records, 0)
        hc = _host_counters(dev)
        hc.arm(ba)
        StageTimer.mark("bin_count")
        N.check(lib.gs_bin_count(C.byref(ba), s), "gs_bin_count")
        image, alpha, depth = _pixel_outputs(H, W, dev)
        # the tile workspace too, at a capacity guessed from the last frame on
        # this device, and the emission queued into it before the sync (it
        # drops entries past the capacity): its kernel time hides the
        # read-back's round trip.  T above the guess: re-allocate, re-emit.
        cap = _capacity_guess(dev)
        if cap:
            fr.tile_ws, fr._to, sort_bytes = tile_workspace(cap)
        # (M, T) reach the host through pinned memory before the emission is
        # queued, so the host wakes while the GPU still emits: gs_bin_count
        # writes them there itself (_HostCounters) -- or, where the runtime
        # does not map the buffer, a copy in the stream and an event
        ready = None
        if hc.dptr is None:
            hc.t[:4].copy_(fr.counters[:4], non_blocking=True)
            ready = torch.cuda.Event()
            ready.record()
        if cap:
            StageTimer.mark("bin_emit")
            N.check(lib.gs_bin_emit(C.byref(ba), s), "gs_bin_emit")
        StageTimer.mark("~sync")
        M, T, zmin, zmax = hc.wait(dev, ready)  # the one host sync
        if not window_holds(window, zmin, zmax):
            _frame_missed(dev, zmax, T)
            return forward_pipeline(cam, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit,
                                    sh_rest, sh_degree, pair_counts, depth_window_ok=False, need_grad=need_grad,
                                    pix_neval=pix_neval, stage_path=stage_path)
    else:
        M, T = 0, 0
    fr.M, fr.T = M, T

    if M == 0:
        if n > 0:
            _frame_done(dev, T, zmin, zmax)
        image, alpha, depth = _empty_frame_outputs(cam, dev)
        fr.pair_offset.zero_()
        return image, alpha, depth, means2d, conics, radii, vis, fr

    # Between the host sync and the blend launch the GPU idles: this span
    # only fills T into the launches (re-emitting first when T exceeded the
    # guess).
    if fr.tile_ws is None or fb.capacity < T:
        fr.tile_ws, fr._to, sort_bytes = tile_workspace(T)
        StageTimer.mark("bin_emit")
        N.check(lib.gs_bin_emit(C.byref(ba), s), "gs_bin_emit")
    to, tw = fr._to, fb.tile_ws
    G = fr.groups = cam.frame_groups(T)  # (from T alone: the gradients' summation order)
    assert G * T <= fb.capacity * fb.flag_groups
    alt = C.c_int32(0)
    StageTimer.mark("tile_sort")
    N.check(lib.gs_radix_sort_pairs(tw + to.tk0, tw + to.tv0, tw + to.tk1, tw + to.tv1, T, 0, bits, 0, tw + to.sort_ws,
                                    sort_bytes, C.byref(alt), s), "tile sort")
    fr.tile_alt = alt.value
    # (with gradients to come: the backward's slot flags zeroed in the same kernel)
    ra = N.GsRangeArgs(T, num_tiles, tw + (to.tk1 if alt.value else to.tk0), fw + fo.ranges,
                       tw + to.flags if need_grad else None, G)
    fr.flags_zeroed = bool(need_grad)
    StageTimer.mark("tile_ranges")
    N.check(lib.gs_tile_ranges(C.byref(ra), s), "gs_tile_ranges")

    fa = N.GsBlendFwdArgs(cs, cam.tiles_x, cam.tiles_y, fw + fo.ranges, tw + (to.tv1 if alt.value else to.tv0),
                          fw + fo.records, N.ptr(image), N.ptr(alpha), N.ptr(depth), fw + fo.pix_flags,
                          fw + fo.cell_neval, tw + to.live if fb.live_cells else None, to.live_words,
                          N.ptr(pair_counts), T, N.ptr(pix_neval))
    StageTimer.mark("blend_fwd")
    N.check(lib.gs_blend_forward(C.byref(fa), s), "gs_blend_forward")
    StageTimer.mark("~end_fwd")
    _frame_done(dev, T, zmin, zmax)  # (the next frame's guesses: after the launches)
    return image, alpha, depth, means2d, conics, radii, vis, fr


def backward_pipeline(cam: CameraParams, fr: _Frame, xyz, cov3d, scaling, rotation, logits, opacity,
                      means2d, conics, g_image, g_alpha, g_depth, g_means2d, g_conics, opacity_is_logit=False,
                      sh_rest=None, sh_degree=0, out=None, outputs=None, d_view=None, feat=None, density=None,
                      dist=None):
    """dist: optional _DistortionGrad with a cotangent on the distortion map (a
    stage-path frame): its geometry, opacity and depth sums are added to the
    colour pass's (and the feature pass's) before the one projection backward.
    density: optional (DensityStats, the forward's radii): the view is added
    to the statistics after the projection backward's last row range.
    outputs: the forward's (image, alpha, depth), unmodified -- with the
    frame's clamp flags they are the blend backward's per-pixel state.
    feat: optional _FeaturePass with a cotangent on the feature image (a
    stage-path frame): its chunks' geometry sums are added to the colour
    pass's before the one projection backward, and feat.d_features is set.
    d_view: optional fp32 [12] on the device -- the projection backward then
    runs as gs_project_backward_pose, one range over every Gaussian, and
    writes dL/d(view rows [R | t]) there (the per-Gaussian gradients are the
    same bits either way).
    out: optional preallocated gradient tensors {name: tensor} (the
    data-parallel bucket's views, distributed.GradAllReduce.attach); the
    kernels write there instead of into fresh buffers.  out["_rows_ready"]
    (optional): called with (lo, hi) once the gradient rows of Gaussians
    [lo, hi) are queued, the last stage running in out["_chunks"] ranges so
    that a range's all-reduce overlaps the next range's kernels."""
    if fr.calls:
        return _backward_frame(cam, fr, xyz, cov3d, scaling, rotation, logits, opacity, means2d, conics, g_image,
                               g_alpha, g_depth, g_means2d, g_conics, opacity_is_logit, sh_rest, sh_degree, out,
                               outputs, d_view, density)
    lib = N.load()
    dev = xyz.device
    n = int(xyz.shape[0])
    f32 = torch.float32
    s = _stream()
    cs = cam.to_struct()
    abs_sums = None
    sums = _GradSums(fr, n, dev)  # (the one owner of this backward's per-Gaussian sums)
    # (statistics with abs_accum: the blend backward also writes the absolute partials, summed
    # per Gaussian right after each batch -- before the flags are cleared or another pass sets its own)
    want_abs = density is not None and density[0].abs_accum is not None
    pixel_grads = g_image is not None or g_alpha is not None or g_depth is not None
    if fr.M > 0 and fr.T > 0 and pixel_grads:
        g_image, g_alpha, g_depth, image, alpha, depth = _pixel_cotangents(cam, g_image, g_alpha, g_depth, outputs,
                                                                           dev)
        # one partial per (slot, cell of the batch) -- per slot at the default
        # tile, whose cells are combined on chip; only replayed entries write
        # theirs and set its flag.  Other tiles' cells run in batches of
        # fr.groups (one batch unless the partials would exceed
        # PARTIAL_BUDGET_BYTES), each summed by gs_gather_partials in order.
        G, Q = fr.groups, cam.cells
        pair_grads = torch.empty((fr.T * G, N.GS_PARTIAL_STRIDE), dtype=f32, device=dev)
        slot_live = fr.slot_live
        if not fr.flags_zeroed:
            # no gs_tile_ranges zeroed them, or a backward of the frame ran
            # before (retain_graph): the flags hold its last batch's, in that
            # batch's layout
            slot_live.zero_()
        fr.flags_zeroed = False
        ba = N.GsBlendBwdArgs(cs, cam.tiles_x, cam.tiles_y, N.ptr(fr.ranges), N.ptr(fr.sorted_gauss),
                              N.ptr(fr.records), N.ptr(image), N.ptr(alpha), N.ptr(depth),
                              N.ptr(fr.pix_flags), N.ptr(fr.cell_neval), N.ptr(g_image), N.ptr(g_alpha), N.ptr(g_depth), N.ptr(fr.live_bits),
                              _live_words(fr), N.ptr(pair_grads),
                              N.ptr(slot_live), fr.T, 0, 0)
        if want_abs:
            abs_grads = torch.empty((fr.T * G, 2), dtype=f32, device=dev)
            abs_sums = torch.empty((n, 2), dtype=f32, device=dev)
            aga = N.GsAbsGatherArgs(n, N.ptr(fr.vis), N.ptr(fr.rects), N.ptr(fr.pair_offset), N.ptr(abs_grads),
                                    N.ptr(slot_live), G, 0, N.ptr(abs_sums))

        def blend_backward(batch: int) -> None:
            if not want_abs:
                N.check(lib.gs_blend_backward(C.byref(ba), s), "gs_blend_backward")
                return
            N.check(lib.gs_blend_backward_abs(C.byref(ba), N.ptr(abs_grads), s), "gs_blend_backward_abs")
            aga.partial_groups, aga.accumulate = ba.cell_count or G, 1 if batch else 0
            N.check(lib.gs_gather_abs_partials(C.byref(aga), s), "gs_gather_abs_partials")

        sums.partials = pair_grads
        if G < cam.groups:
            ga = sums.gather_args(pair_grads, slot_live)
            for b, c0 in enumerate(range(0, Q, G)):
                ba.cell_begin, ba.cell_count = c0, min(G, Q - c0)
                if b:
                    slot_live.zero_()
                blend_backward(b)
                sums.gather(lib, ga, ba.cell_count, s)
        else:
            StageTimer.mark("blend_bwd")
            blend_backward(0)
            sums.flags = slot_live  # (one batch: left as partials, for the next pass or the projection to sum)
    grads, rows_ready, chunks = _grad_buffers(out, n, cov3d is None, sh_degree, dev)
    d_xyz, d_cov, d_scl, d_rot, d_col, d_op, d_sh = grads
    gm = None if g_means2d is None else g_means2d.contiguous()
    gc = None if g_conics is None else g_conics.contiguous()
    gst = _gaussians_struct(n, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit, sh_rest, sh_degree)
    # (the colour pass's sums first, then every feature chunk's and the distortion's added:
    # one projection backward over the total)
    if feat is not None and fr.M > 0 and fr.T > 0:
        _feature_backward(lib, cam, fr, feat, sums, s)
    if dist is not None and fr.M > 0 and fr.T > 0:
        _distortion_backward(lib, cam, fr, dist, sums, s)
    pair_grads, slot_live, grad_sums = sums.for_projection()
    pb = N.GsProjectBwdArgs(cs, gst, N.ptr(means2d), N.ptr(conics), N.ptr(fr.vis), N.ptr(fr.rects),
                            # Gaussian order (order=NULL): inputs/outputs stream; walking in depth
                            # order coalesces the slot reads but scatters 10 arrays (measured 2.4x slower)
                            N.ptr(fr.pair_offset), None, N.ptr(pair_grads), N.ptr(gm), N.ptr(gc), N.ptr(d_xyz),
                            N.ptr(d_cov), N.ptr(d_scl), N.ptr(d_rot), N.ptr(d_col), N.ptr(d_op), N.ptr(d_sh),
                            N.ptr(slot_live), N.ptr(grad_sums), fr.groups, cam.filter_struct())
    StageTimer.mark("project_bwd")
    _project_backward_ranges(lib, pb, n, chunks, rows_ready, d_view, s)
    if density is not None:
        _accumulate_density(lib, cam, density[0], n, fr.vis, density[1], N.ptr(grad_sums) or None, gm, s,
                            abs_sums)
    StageTimer.mark("~end_bwd")
    return grads


def _pixel_cotangents(cam: CameraParams, g_image, g_alpha, g_depth, outputs, dev):
    """The blend backward's per-pixel inputs when any pixel cotangent is
    given: the three cotangents contiguous (a missing g_image as zeros), then
    the forward's image, alpha, depth (_blend_outputs)."""
    if g_image is None:
        g_image = torch.zeros((3, cam.image_height, cam.image_width), dtype=torch.float32, device=dev)
    g_image = g_image.contiguous()
    g_alpha = None if g_alpha is None else g_alpha.contiguous()
    g_depth = None if g_depth is None else g_depth.contiguous()
    return (g_image, g_alpha, g_depth, *_blend_outputs(outputs))


def _grad_buffers(out, n: int, raw: bool, sh_degree: int, dev):
    """((d_xyz, d_cov, d_scl, d_rot, d_col, d_op, d_sh), rows_ready, chunks):
    the projection backward's gradient tensors -- the caller's from `out`
    (backward_pipeline), viewed to the kernels' shapes, fresh ones otherwise --
    and out's "_rows_ready" callback with its "_chunks" (1 without a callback).
    raw: scaling / rotation inputs (their gradients, no d_cov)."""
    out = dict(out or {})
    rows_ready = out.pop("_rows_ready", None)
    chunks = int(out.pop("_chunks", 1)) if rows_ready is not None else 1
    f32 = torch.float32

    def buf(name, shape):
        t = out.get(name)
        return t.view(shape) if t is not None else torch.empty(shape, dtype=f32, device=dev)
    d_xyz = buf("xyz", (n, 3))
    d_cov = None if raw else torch.empty((n, 3, 3), dtype=f32, device=dev)
    d_scl = buf("scaling", (n, 3)) if raw else None
    d_rot = buf("rotation", (n, 4)) if raw else None
    d_col = buf("color", (n, 3))
    d_op = buf("opacity", (n,))
    d_sh = buf("sh_rest", (n, N.GS_SH_REST, 3)) if sh_degree > 0 else None
    return (d_xyz, d_cov, d_scl, d_rot, d_col, d_op, d_sh), rows_ready, chunks


def _project_backward_ranges(lib, pb: "N.GsProjectBwdArgs", n: int, chunks: int, rows_ready, d_view, s) -> None:
    """The projection backward of `pb`'s n Gaussians: with d_view one
    gs_project_backward_pose over all of them (the pose gradient's reduction
    wants one range), else gs_project_backward per row range of `chunks`,
    rows_ready(lo, hi) called as soon as a range's rows are queued (its
    all-reduce then overlaps the next range's kernels)."""
    if d_view is not None:
        _project_backward_pose(lib, pb, n, d_view, s)
        if rows_ready is not None:
            rows_ready(0, n)
        return
    bounds = [n * k // chunks for k in range(chunks + 1)]
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        part = pb if (lo, hi) == (0, n) else _rows_of(pb, lo, hi)
        N.check(lib.gs_project_backward(C.byref(part), s), "gs_project_backward")
        if rows_ready is not None:
            rows_ready(lo, hi)


def _project_backward_pose(lib, pb: "N.GsProjectBwdArgs", n: int, d_view: torch.Tensor, s) -> None:
    """gs_project_backward_pose over every Gaussian of `pb`: the projection
    backward plus the deterministic two-level sum of the pose gradient (one
    row of partials per workgroup of GS_POSE_BLOCK Gaussians)."""
    rows = max(1, (n + N.GS_POSE_BLOCK - 1) // N.GS_POSE_BLOCK)
    partials = torch.empty((rows, N.GS_POSE_ROW), dtype=torch.float64, device=d_view.device)
    pa = N.GsProjectPoseArgs(pb, partials.data_ptr(), rows, d_view.data_ptr())
    N.check(lib.gs_project_backward_pose(C.byref(pa), s), "gs_project_backward_pose")


def _blend_outputs(outputs):
    """The forward's image, alpha, depth as the blend backward reads them
    (fp32, contiguous, as rasterize returned them)."""
    if outputs is None:
        raise ValueError("the blend backward needs the forward's (image, alpha, depth)")
    image, alpha, depth = outputs
    for t in (image, alpha, depth):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise ValueError("the forward's image / alpha / depth must be the contiguous fp32 tensors it returned")
    return image, alpha, depth


def _backward_frame(cam: CameraParams, fr: _Frame, xyz, cov3d, scaling, rotation, logits, opacity, means2d,
                    conics, g_image, g_alpha, g_depth, g_means2d, g_conics, opacity_is_logit, sh_rest, sh_degree, out,
                    outputs, d_view=None, density=None):
    """backward_pipeline through gs_render_backward (the frame of
    _forward_frame): the blend backward and the gather in the library, then
    the projection backward -- there too unless the data-parallel reduction
    wants the rows in ranges, or the pose gradient is wanted (d_view)."""
    lib = N.load()
    dev = xyz.device
    n = int(xyz.shape[0])
    f32 = torch.float32
    s = _stream()
    pixel_grads = g_image is not None or g_alpha is not None or g_depth is not None
    ba = N.GsRenderBwdArgs()
    ba.cam, ba.fb, ba.M, ba.T, ba.tile_alt = fr.cam, fr.fb, fr.M, fr.T, fr.tile_alt
    # (the forward's Gaussians: the tensors autograd saved for this backward)
    ba.g = _gaussians_struct(n, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit, sh_rest, sh_degree)
    ba.means2d, ba.conics, ba.vis = N.ptr(means2d), N.ptr(conics), N.ptr(fr.vis)
    if cam.screen_filter:  # (ba is zeroed: no filter)
        ba.filter = cam.filter_struct()
    pair_grads = None
    if fr.M > 0 and fr.T > 0 and pixel_grads:
        g_image, g_alpha, g_depth, image, alpha, depth = _pixel_cotangents(cam, g_image, g_alpha, g_depth, outputs,
                                                                           dev)
        pair_grads = torch.empty((fr.T * fr.groups, N.GS_PARTIAL_STRIDE), dtype=f32, device=dev)
        ba.image, ba.alpha, ba.depth = image.data_ptr(), alpha.data_ptr(), depth.data_ptr()
        ba.g_image, ba.g_alpha, ba.g_depth = N.ptr(g_image), N.ptr(g_alpha), N.ptr(g_depth)
        ba.pair_grads = pair_grads.data_ptr()
        ba.flags_zeroed = 1 if fr.flags_zeroed else 0
        fr.flags_zeroed = False  # (a second backward of the frame clears its flags first: ADVICE r05)
    gm = None if g_means2d is None else g_means2d.contiguous()
    gc = None if g_conics is None else g_conics.contiguous()
    ba.g_means2d, ba.g_conics = N.ptr(gm), N.ptr(gc)
    grads, rows_ready, chunks = _grad_buffers(out, n, cov3d is None, sh_degree, dev)
    d_xyz, d_cov, d_scl, d_rot, d_col, d_op, d_sh = grads
    ba.d_xyz, ba.d_cov3d, ba.d_scaling, ba.d_rotation = N.ptr(d_xyz), N.ptr(d_cov), N.ptr(d_scl), N.ptr(d_rot)
    ba.d_color_logits, ba.d_opacity, ba.d_sh_rest = N.ptr(d_col), N.ptr(d_op), N.ptr(d_sh)
    ba.project = 1 if (chunks == 1 and d_view is None) else 0
    ev = StageTimer.pair("blend_bwd")
    if ev is not None:
        ba.blend_events[0], ba.blend_events[1] = ev[0].handle, ev[1].handle
    N.check(lib.gs_render_backward(C.byref(ba), s), "gs_render_backward")
    # (the gathered sums in the frame workspace, when this backward had a blend gradient)
    sums = ba.grad_sums if pair_grads is not None else None
    if ba.project:
        if rows_ready is not None:
            rows_ready(0, n)
        if density is not None:
            _accumulate_density(lib, cam, density[0], n, fr.vis, density[1], sums, gm, s)
        return grads
    # the projection backward from here: per row range, each range's
    # reduction issued as soon as its rows are queued, or with the pose gradient
    fo, fws = fr.fo, fr.frame_ws.data_ptr()
    pb = N.GsProjectBwdArgs(fr.cam, ba.g, ba.means2d, ba.conics, ba.vis, fws + fo.rects, fws + fo.pair_offset, None,
                            None, N.ptr(gm),
                            N.ptr(gc), N.ptr(d_xyz), N.ptr(d_cov), N.ptr(d_scl), N.ptr(d_rot), N.ptr(d_col),
                            N.ptr(d_op), N.ptr(d_sh), None, sums, 0, ba.filter)
    _project_backward_ranges(lib, pb, n, chunks, rows_ready, d_view, s)
    if density is not None:
        _accumulate_density(lib, cam, density[0], n, fr.vis, density[1], sums, gm, s)
    return grads


def _rows_of(pb: "N.GsProjectBwdArgs", lo: int, hi: int) -> "N.GsProjectBwdArgs":
    """The projection backward's arguments restricted to Gaussians [lo, hi):
    every per-Gaussian pointer advanced by lo rows (the slot partials are
    addressed through pair_offset, absolute, and stay)."""
    r = N.GsProjectBwdArgs.from_buffer_copy(pb)
    g = r.g

    def adv(ptr, row_bytes):
        return ptr + lo * row_bytes if ptr else ptr
    g.n = hi - lo
    g.xyz = adv(g.xyz, 4 * g.xyz_stride)
    g.cov3d = adv(g.cov3d, 36)
    g.scaling = adv(g.scaling, 12)
    g.rotation = adv(g.rotation, 16)
    g.color_logits = adv(g.color_logits, 4 * g.color_stride)
    g.opacity = adv(g.opacity, 4 * g.opacity_stride)
    g.sh_rest = adv(g.sh_rest, 4 * g.sh_rest_stride)
    for name, rb in (("means2d", 8), ("conics", 16), ("vis", 1), ("rects", 8), ("pair_offset", 4),
                     ("g_means2d", 8), ("g_conics", 16), ("d_xyz", 12), ("d_cov3d", 36), ("d_scaling", 12),
                     ("d_rotation", 16), ("d_color_logits", 12), ("d_opacity", 4),
                     ("d_sh_rest", 4 * N.GS_SH_REST * 3), ("grad_sums", 4 * N.GS_PAIR_GRAD_FLOATS)):
        setattr(r, name, adv(getattr(r, name), rb))
    if r.order:
        raise ValueError("row ranges need the Gaussian-order walk (order = NULL)")
    return r


class _FeaturePass:
    """One backward's view of a frame's feature pass: the staged input, the
    forward's feature image, its cotangent, and the result d_features [n, C]."""
    __slots__ = ("staged", "out", "g_out", "channels", "d_features")

    def __init__(self, staged, out, g_out, channels):
        self.staged, self.out, self.g_out, self.channels, self.d_features = staged, out, g_out, channels, None


def _feature_chunks(channels: int) -> int:
    return (channels + N.GS_FEATURE_CHUNK - 1) // N.GS_FEATURE_CHUNK


def _stage_features(features: torch.Tensor) -> torch.Tensor:
    """[n, C] fp32 -> [ceil(C/4), n, 4] contiguous, the last chunk zero-padded:
    the kernels read a chunk's payload as one aligned 16-byte load per entry
    (rows of a [n, C] tensor are 16-byte aligned only when C % 4 == 0, and a
    chunk's rows would be C floats apart).  A torch pad + transpose copy."""
    n, c = features.shape
    k = _feature_chunks(c)
    f = features.detach()
    if c != k * N.GS_FEATURE_CHUNK:
        f = torch.nn.functional.pad(f, (0, k * N.GS_FEATURE_CHUNK - c))
    return f.reshape(n, k, N.GS_FEATURE_CHUNK).permute(1, 0, 2).contiguous()


def _feature_forward(cam: CameraParams, fr: _Frame, staged: torch.Tensor, channels: int, n: int, dev) -> torch.Tensor:
    """The feature image [C, H, W] of a stage-path frame: gs_blend_features_forward
    over the state the colour forward left in `fr` (zeros when nothing was drawn)."""
    H, W = int(cam.image_height), int(cam.image_width)
    if fr.M == 0 or fr.T == 0:
        return torch.zeros((channels, H, W), dtype=torch.float32, device=dev)
    out = torch.empty((channels, H, W), dtype=torch.float32, device=dev)
    fa = N.GsFeatureFwdArgs(replay_frame(cam, fr, n), channels, N.ptr(staged), N.ptr(out))
    StageTimer.mark("features_fwd")
    N.check(N.load().gs_blend_features_forward(C.byref(fa), _stream()), "gs_blend_features_forward")
    StageTimer.mark("~end_features_fwd")
    return out


def _feature_backward(lib, cam: CameraParams, fr: _Frame, feat: _FeaturePass, sums: _GradSums, s) -> None:
    """The feature pass's backward over a stage-path frame: per chunk and cell
    batch (the frame's own plan: fr.groups cells at a time) the blend backward
    of that chunk and its gather -- geometry sums added to `sums`, the chunk's
    columns of feat.d_features stored by a chunk's first batch and added to by
    the later ones."""
    n, f32 = sums.n, torch.float32
    G, Q, Cn = fr.groups, cam.cells, feat.channels
    pair_grads, flags = sums.scratch(lib, s)
    g_out = _fp32_contiguous(feat.g_out)
    d_features = torch.empty((n, Cn), dtype=f32, device=sums.dev)
    ba = N.GsFeatureBwdArgs(replay_frame(cam, fr, n), Cn, 0, N.ptr(feat.staged), N.ptr(feat.out), N.ptr(g_out),
                            N.ptr(pair_grads), N.ptr(flags), 0, 0)
    fg = N.GsFeatureGatherArgs(n, N.ptr(fr.vis), N.ptr(fr.rects), N.ptr(fr.pair_offset), N.ptr(pair_grads),
                               N.ptr(flags), G, 0, N.ptr(sums.sums), N.ptr(d_features), d_features.stride(0), 0, 0, 0)
    StageTimer.mark("features_bwd")
    for chunk in range(_feature_chunks(Cn)):
        ba.chunk = chunk
        fg.channel_begin = chunk * N.GS_FEATURE_CHUNK
        fg.channel_count = min(N.GS_FEATURE_CHUNK, Cn - fg.channel_begin)
        for b, c0 in enumerate(range(0, Q, G)):
            ba.cell_begin, ba.cell_count = c0, min(G, Q - c0)
            fg.partial_groups = ba.cell_count
            fg.accumulate, fg.feature_accumulate = sums.accumulate(), (1 if b else 0)
            flags.zero_()
            N.check(lib.gs_blend_features_backward(C.byref(ba), s), "gs_blend_features_backward")
            N.check(lib.gs_gather_feature_partials(C.byref(fg), s), "gs_gather_feature_partials")
    StageTimer.mark("~end_features_bwd")
    feat.d_features = d_features


class RasterizeGaussians(torch.autograd.Function):
    """Differentiable render: inputs are the model accessors' tensors, outputs
    are (image, alpha, depth, viewspace_points, conics, radii, visibility),
    then the feature image [C, H, W] when `features` [N, C] were given (one
    more differentiable input, composited with the colour pass's own weights),
    then the distortion map when `distort` asks for it."""

    @staticmethod
    def forward(ctx, xyz, cov3d, scaling, rotation, logits, opacity, sh_rest, features, view, cam: CameraParams,
                opacity_is_logit=False, sh_degree=0, grad_dest=None, density_stats=None, contrib=None, distort=None):
        # features, contrib (a _ContributionPass), distort (a _DistortionPass), density_stats with
        # abs_accum (its backward is gs_blend_backward_abs): the frame is then the stage path's, whose
        # buffers the replays read -- the seven standard outputs and their gradients are the same bits;
        # the contribution pass runs at the end of this forward
        # density_stats: a DensityStats this frame's backward adds the view to (it needs the
        # forward's radii, kept on ctx: a non-differentiable output, no cycle through the tape)
        # view: None, or the camera's W2C rows as an fp32 [3,4] / [4,4] tensor on the
        # Gaussians' device, given only to receive its gradient -- the forward
        # reads the pose from `cam`, whose values are the same
        image, alpha, depth, means2d, conics, radii, vis, fr = forward_pipeline(
            cam, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit, sh_rest, sh_degree,
            need_grad=_FUSE_FLAGS and any(ctx.needs_input_grad[:7]),
            stage_path=features is not None or contrib is not None or distort is not None or
            (density_stats is not None and density_stats.abs_accum is not None))
        n, dev = int(xyz.shape[0]), xyz.device
        extra = ()
        ctx.feature_shape = None if features is None else (n, int(features.shape[1]))
        if features is not None:
            staged = _stage_features(features)
            extra = (staged, _feature_forward(cam, fr, staged, ctx.feature_shape[1], n, dev))
        if distort is not None:
            extra += (_distortion_forward(cam, fr, n, distort, dev),)
        if contrib is not None:
            _contribution_pass(cam, fr, n, contrib, dev)
        ctx.cam, ctx.frame, ctx.opacity_is_logit, ctx.sh_degree = cam, fr, opacity_is_logit, sh_degree
        ctx.grad_dest = grad_dest
        ctx.distort = distort
        ctx.density = None if density_stats is None else (density_stats, radii)
        ctx.view_shape = tuple(view.shape) if view is not None and ctx.needs_input_grad[8] else None
        # (the outputs image / alpha / depth too: the blend backward's per-pixel
        # state; autograd refuses the backward if they were modified in place)
        ctx.save_for_backward(xyz, cov3d, scaling, rotation, logits, opacity, sh_rest, means2d, conics, image, alpha,
                              depth, *extra)
        ctx.mark_non_differentiable(radii, vis)
        ctx.set_materialize_grads(False)
        return (image, alpha, depth, means2d, conics, radii, vis) + extra[1 if features is not None else 0:]

    @staticmethod
    def backward(ctx, g_image, g_alpha, g_depth, g_means2d, g_conics, _g_radii, _g_vis, *g_extra):
        (xyz, cov3d, scaling, rotation, logits, opacity, sh_rest, means2d, conics, image, alpha, depth,
         *extra) = ctx.saved_tensors
        g_extra = list(g_extra)
        # (no cotangent on the feature image or the distortion map: no launch for it)
        feat = dist = None
        if ctx.feature_shape is not None:
            staged, feat_image, g_features = extra[0], extra[1], g_extra.pop(0)
            if g_features is not None:
                feat = _FeaturePass(staged, feat_image, g_features, ctx.feature_shape[1])
        if ctx.distort is not None and g_extra[0] is not None:
            dist = _DistortionGrad(ctx.distort, extra[-1], g_extra[0])
        g_conics = None if g_conics is None else g_conics.reshape(-1, 4)
        dest = ctx.grad_dest() if ctx.grad_dest is not None else None
        d_view = None
        if ctx.view_shape is not None:
            d_view = torch.empty((12,), dtype=torch.float32, device=xyz.device)
        d_xyz, d_cov, d_scl, d_rot, d_col, d_op, d_sh = backward_pipeline(
            ctx.cam, ctx.frame, xyz, cov3d, scaling, rotation, logits, opacity, means2d, conics,
            g_image, g_alpha, g_depth, g_means2d, g_conics, ctx.opacity_is_logit,
            sh_rest, ctx.sh_degree, out=dest, outputs=(image, alpha, depth), d_view=d_view, feat=feat,
            density=ctx.density, dist=dist)
        need = ctx.needs_input_grad
        d_features = None
        if need[7] and feat is not None:
            d_features = feat.d_features
            if d_features is None:  # (nothing drawn: no entry carries the cotangent anywhere)
                d_features = torch.zeros(ctx.feature_shape, dtype=torch.float32, device=xyz.device)
        g_view = None
        if d_view is not None:
            g_view = d_view.view(3, 4)
            if ctx.view_shape == (4, 4):
                g_view = torch.cat([g_view, g_view.new_zeros((1, 4))], 0)
        return (d_xyz if need[0] else None,
                d_cov if (cov3d is not None and need[1]) else None,
                d_scl if (scaling is not None and need[2]) else None,
                d_rot if (rotation is not None and need[3]) else None,
                d_col.view(logits.shape) if need[4] else None,
                d_op.view(opacity.shape) if need[5] else None,
                d_sh if (sh_rest is not None and need[6]) else None,
                d_features, g_view, None, None, None, None, None, None, None)


def rasterize(cam: CameraParams, xyz, cov3d, scaling, rotation, logits, opacity, opacity_is_logit=False,
              sh_rest=None, sh_degree=0, grad_dest=None, view=None, features=None, density_stats=None,
              contribution_stats=None, dominant=False, depth_distortion=False, distortion_near_far=None):
    """depth_distortion=True: three more outputs follow (after the feature
    image, when there is one, and before the dominant maps): the fp32 [H, W]
    depth distortion sum_i sum_j c_i c_j |m_i - m_j| of each pixel's
    contributors (gs_blend_distortion_forward; differentiable in the geometry,
    the opacity and, through d_z and the weights, `view`), the fp32 [H, W]
    median depth and the int32 [H, W] median Gaussian (-1: none), neither with
    a gradient.  m is the camera-space depth, or with
    distortion_near_far=(near, far) 2DGS's inverse (NDC) depth; a bad pair, or
    one without depth_distortion, is a ValueError before any launch.  The frame
    takes the stage path (the seven standard outputs and their gradients are
    the same bits); the distortion's backward runs only when the map received
    a cotangent, and density_stats then see the summed dL/dmeans2d, the
    distortion's part included.
    contribution_stats: optional ContributionStats of N Gaussians on their
    device (checked here, before any launch): the forward ends with the
    contribution pass, which adds this view's per-Gaussian blend weights to
    it (sum, max, pixel count, views).  dominant=True: two more outputs follow
    (after the feature image, when there is one): the int32 [H, W] id of
    each pixel's strongest contributor (-1: none) and its fp32 weight.
    Neither needs a backward; both take the stage path, whose seven standard
    outputs and gradients are the same bits.
    density_stats: optional DensityStats of N Gaussians on their device: the
    backward of this render ends with one gs_density_accumulate that adds the
    view to it (checked here, before any launch; see DensityStats for what a
    missing or repeated backward means).  Without it the launches are the same.
    DensityStats(abs_grad=True) take the stage path (the same outputs and
    gradients, bit for bit) and also accumulate the absolute screen-space
    gradient of the colour pass, abs_accum (gs_blend_backward_abs,
    gs_gather_abs_partials, gs_density_accumulate_abs in place of the signed
    launch); feature and distortion passes add to the signed sums only.
    features: optional floating-point [N, C] tensor on the Gaussians' device,
    C in 1..GS_MAX_FEATURE_CHANNELS: an eighth output follows the seven, the
    feature image [C, H, W] fp32 = sum_i c_i features[g_i] per pixel with the
    colour pass's own weights c_i (no background, clamp or normalisation);
    differentiable in the features and in the geometry (and `view`).
    opacity_is_logit: opacity holds the model's raw _opacity and the kernels
    apply get_opacity's sigmoid (fused; its gradient goes to the logit).
    sh_degree > 0: view-dependent colour from sh_rest ([N,15,3] rest
    coefficients, e.g. get_features[:,1:,:]); 0 is the reference's DC-only
    colour (include/gsplat_mi355x.h, gs_gaussians).
    grad_dest: optional callable, asked at backward time, returning None or
    {name: tensor} buffers the gradient kernels write into (names xyz,
    scaling, rotation, color, opacity, sh_rest; see backward_pipeline).
    view: optional [3,4] or [4,4] floating-point tensor, the world-to-camera
    matrix whose rows cam.view holds, on any device: when it requires grad it
    receives dL/d(view) (in its own dtype, on its own device; row 3 of a 4x4
    is zero).  The forward's values come from `cam` either way."""
    _check_inputs(xyz)
    n = int(xyz.shape[0]) if xyz.dim() == 2 else -1
    if n < 0 or xyz.shape[1] != 3:
        raise ValueError(f"xyz must be [N, 3], got {tuple(xyz.shape)}")

    def prep(name, t, tail):
        """Same device as xyz, N rows of `tail` trailing shape, fp32 (other
        float dtypes are cast, the cast on the autograd tape): the kernels read
        raw fp32 rows, so anything else would be read as garbage."""
        if t is None:
            return None
        if t.device != xyz.device:
            raise RuntimeError(f"{name} is on {t.device}, the Gaussians' xyz on {xyz.device}")
        if not t.is_floating_point():
            raise TypeError(f"{name} must be a floating-point tensor, got {t.dtype}")
        if t.dim() == 0 or t.shape[0] != n or t.numel() != n * math.prod(tail):
            raise ValueError(f"{name} must hold {list(tail)} per Gaussian for N = {n}, got {tuple(t.shape)}")
        return t if t.dtype == torch.float32 else t.float()

    if density_stats is not None:
        _check_density_stats(density_stats, n, xyz.device)
    if contribution_stats is not None:
        _check_contribution_stats(contribution_stats, n, xyz.device)
    if distortion_near_far is not None and not depth_distortion:
        raise ValueError("distortion_near_far needs depth_distortion=True")
    dp = _DistortionPass(distortion_near_far) if depth_distortion else None
    xyz = prep("xyz", xyz, (3,))
    cov3d = prep("cov3d", cov3d, (3, 3))
    scaling = prep("scaling", scaling, (3,))
    rotation = prep("rotation", rotation, (4,))
    logits = prep("colour", logits, (3,))
    opacity = prep("opacity", opacity, (1,))
    if features is not None:
        if not isinstance(features, torch.Tensor):
            raise TypeError(f"features must be a tensor, got {type(features).__name__}")
        if features.dim() != 2:
            raise ValueError(f"features must be [N, C], got {tuple(features.shape)}")
        if not 1 <= features.shape[1] <= N.GS_MAX_FEATURE_CHANNELS:
            raise ValueError(f"features must have 1..{N.GS_MAX_FEATURE_CHANNELS} channels "
                             f"(GS_MAX_FEATURE_CHANNELS), got {features.shape[1]}")
        features = prep("features", features, (features.shape[1],))
    if cov3d is None and (scaling is None or rotation is None):
        raise ValueError("need a covariance or scaling + rotation")
    sh_degree = int(sh_degree)
    if not 0 <= sh_degree <= 3:
        raise ValueError(f"sh_degree must be in 0..3, got {sh_degree}")
    if sh_degree > 0:
        if sh_rest is None or tuple(sh_rest.shape[1:]) != (N.GS_SH_REST, 3):
            raise ValueError("sh_degree > 0 needs sh_rest of shape [N, 15, 3]")
        sh_rest = prep("sh_rest", sh_rest, (N.GS_SH_REST, 3))
        if sh_rest.stride(2) != 1 or sh_rest.stride(1) != 3:
            sh_rest = sh_rest.contiguous()
    else:
        sh_rest = None
    if cov3d is not None:
        cov3d = cov3d.reshape(-1, 3, 3)
        if not cov3d.is_contiguous():
            cov3d = cov3d.contiguous()
    else:
        scaling = scaling.contiguous()
        rotation = rotation.contiguous()
    xyz, _ = _rows(xyz, 3)
    logits, _ = _rows(logits, 3)
    opacity, _ = _rows(opacity, 1)
    cp = _ContributionPass(contribution_stats, dominant) if (contribution_stats is not None or dominant) else None
    if view is None or not (isinstance(view, torch.Tensor) and view.requires_grad):
        view = None
    else:
        if not view.is_floating_point() or tuple(view.shape) not in ((3, 4), (4, 4)):
            raise ValueError(f"view must be a floating-point [3,4] or [4,4] tensor, got {view.dtype} "
                             f"{tuple(view.shape)}")
        # (differentiable, as the reference's .to(device): the gradient returns to
        # the caller's device and dtype)
        view = view.to(device=xyz.device, dtype=torch.float32)
    outs = RasterizeGaussians.apply(xyz, cov3d, scaling, rotation, logits, opacity, sh_rest, features, view, cam,
                                    bool(opacity_is_logit), sh_degree, grad_dest, density_stats, cp, dp)
    if dp is not None:
        outs = tuple(outs) + (dp.median_depth, dp.median_id)
    if cp is not None and cp.dominant:
        outs = tuple(outs) + (cp.dominant_id, cp.dominant_weight)
    return outs
