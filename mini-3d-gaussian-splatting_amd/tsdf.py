"""TSDF fusion of rendered depth maps and mesh extraction (the last step of
2DGS, GOF, RaDe-GS and gsplat's 2DGS trainer; not in the reference): render a
depth map per training view, fuse the maps into a truncated signed distance
volume (KinectFusion's / Open3D's z-projective running mean) and extract a
triangle mesh from it with surface nets.  Three HIP entry points
(include/gsplat_mi355x.h, "TSDF fusion and mesh extraction"):

  TSDFVolume.integrate      gs_tsdf_integrate: any number of views of one size
                            in one launch, the node in registers over them
  TSDFVolume.extract_mesh   gs_mesh_classify, two torch.cumsum, one host read of
                            the two totals, gs_mesh_emit

save_mesh_ply writes the result as a binary PLY.  There is no CPU path, and no
gradient flows through the fusion.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import numpy as np
import torch

from . import _native as N
from .filter3d import camera_row

MAX_NODES = 2 ** 31  # Nx Ny Nz must stay below


def _triple(v, what: str, kind):
    ok = isinstance(v, (tuple, list, np.ndarray, torch.Tensor)) and len(v) == 3
    if ok:
        try:
            out = tuple(kind(x) for x in v)
        except (TypeError, ValueError):
            ok = False
    if not ok:
        raise ValueError(f"{what} must hold three numbers, got {v!r}")
    return out


def _check_dims(dims) -> tuple:
    ok = isinstance(dims, (tuple, list)) and len(dims) == 3 and \
        all(isinstance(d, (int, np.integer)) and not isinstance(d, bool) for d in dims)
    if not ok or min(dims) < 1:
        raise ValueError(f"dims must be (Nx, Ny, Nz) integers, each at least 1, got {dims!r}")
    dims = tuple(int(d) for d in dims)
    if dims[0] * dims[1] * dims[2] >= MAX_NODES:
        raise ValueError(f"dims {dims} hold {dims[0] * dims[1] * dims[2]} nodes: a volume must have fewer than 2^31")
    return dims


class TSDFVolume:
    """A truncated signed distance volume of dims = (Nx, Ny, Nz) samples at
    the nodes origin + voxel_size (i, j, k), on `device`: `tsdf` (1 where
    nothing was fused), `weight` (the number of views fused into the node) and,
    with color=True, `color` [3, Nz, Ny, Nx]; the layout is [Nz, Ny, Nx].
    trunc is the truncation distance in world units (None: 4 voxels), near the
    camera-space depth a node must exceed to be seen by a view."""

    def __init__(self, origin, voxel_size: float, dims, device, trunc: Optional[float] = None, color: bool = True,
                 near: float = 0.2):
        self.origin = _triple(origin, "origin", float)
        if not all(math.isfinite(v) for v in self.origin):
            raise ValueError(f"origin must be finite, got {origin!r}")
        if isinstance(voxel_size, bool) or not isinstance(voxel_size, (int, float, np.floating)) or \
                not (math.isfinite(voxel_size) and voxel_size > 0):
            raise ValueError(f"voxel_size must be finite and > 0, got {voxel_size!r}")
        self.voxel_size = float(voxel_size)
        self.dims = _check_dims(dims)
        trunc = 4.0 * self.voxel_size if trunc is None else trunc
        if not (math.isfinite(trunc) and trunc > 0):
            raise ValueError(f"trunc must be finite and > 0, got {trunc!r}")
        if not (math.isfinite(near) and near > 0):
            raise ValueError(f"near must be finite and > 0, got {near!r}")
        self.trunc, self.near = float(trunc), float(near)
        nx, ny, nz = self.dims
        self.tsdf = torch.ones((nz, ny, nx), dtype=torch.float32, device=torch.device(device))
        self.device = self.tsdf.device  # ("cuda" resolved to the current device's index)
        self.weight = torch.zeros((nz, ny, nx), dtype=torch.float32, device=self.device)
        self.color = torch.zeros((3, nz, ny, nx), dtype=torch.float32, device=self.device) if color else None

    @classmethod
    def from_bounds(cls, lo, hi, voxel_size: float, device, **kw) -> "TSDFVolume":
        """The volume whose nodes start at `lo` and reach `hi` on every axis:
        ceil((hi - lo) / voxel_size) + 1 samples."""
        lo, hi = _triple(lo, "lo", float), _triple(hi, "hi", float)
        if not all(math.isfinite(a) and math.isfinite(b) and b >= a for a, b in zip(lo, hi)):
            raise ValueError(f"bounds must be finite with hi >= lo, got {lo!r}, {hi!r}")
        if isinstance(voxel_size, bool) or not isinstance(voxel_size, (int, float, np.floating)) or \
                not (math.isfinite(voxel_size) and voxel_size > 0):
            raise ValueError(f"voxel_size must be finite and > 0, got {voxel_size!r}")
        dims = tuple(int(math.ceil((b - a) / voxel_size - 1e-9)) + 1 for a, b in zip(lo, hi))
        return cls(lo, voxel_size, dims, device, **kw)

    # -- state -------------------------------------------------------------
    def reset(self) -> None:
        self.tsdf.fill_(1.0)
        self.weight.zero_()
        if self.color is not None:
            self.color.zero_()

    def state(self) -> Dict[str, torch.Tensor]:
        st = {"tsdf": self.tsdf, "weight": self.weight}
        if self.color is not None:
            st["color"] = self.color
        return st

    def load_state(self, state: Dict[str, torch.Tensor]) -> None:
        nx, ny, nz = self.dims
        names = [("tsdf", (nz, ny, nx)), ("weight", (nz, ny, nx))] + ([("color", (3, nz, ny, nx))] if self.color is not None else [])
        for name, shape in names:
            t = state.get(name)
            if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape or t.dtype != torch.float32:
                got = f"{t.dtype} {tuple(t.shape)}" if isinstance(t, torch.Tensor) else type(t).__name__
                raise ValueError(f"the volume's {name} must be fp32 {shape}, got {got}")
        for name, _ in names:
            getattr(self, name).copy_(state[name])

    def _vol(self) -> N.GsTsdfVolume:
        nx, ny, nz = self.dims
        return N.GsTsdfVolume(nx, ny, nz, (C.c_float * 3)(*self.origin), self.voxel_size, self.tsdf.data_ptr(),
                              self.weight.data_ptr(), N.ptr(self.color))

    # -- fusion ------------------------------------------------------------
    def _check_map(self, t, name: str, shape: tuple) -> torch.Tensor:
        if not isinstance(t, torch.Tensor) or tuple(t.shape) != shape:
            got = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"integrate: {name} must be {list(shape)}, got {got}")
        if t.dtype != torch.float32:
            raise ValueError(f"integrate: {name} must be fp32, got {t.dtype}")
        if t.device != self.device:
            raise ValueError(f"integrate: {name} is on {t.device}, the volume on {self.device}")
        return t.detach().contiguous()

    @torch.no_grad()
    def integrate(self, depth: torch.Tensor, cameras, alpha: Optional[torch.Tensor] = None,
                  image: Optional[torch.Tensor] = None, alpha_min: float = 0.5,
                  depth_max: float = math.inf) -> None:
        """Fuse depth maps into the volume, one launch: `depth` [H, W] with one
        camera, or [V, H, W] with a list of V cameras (fused in list order);
        optionally `alpha` of the depth's shape and `image` [3, H, W] /
        [V, 3, H, W].  A node is updated by a view when it projects (to the
        nearest pixel) onto a pixel with 0 < depth <= depth_max and alpha >=
        alpha_min and lies no further than trunc behind that depth:
        tsdf and colour become running means over the views, weight counts
        them.  fp32 tensors on the volume's device; each camera's size must be
        the maps'.  Anything else is a ValueError before any launch."""
        if not isinstance(depth, torch.Tensor) or depth.dim() not in (2, 3):
            got = tuple(depth.shape) if isinstance(depth, torch.Tensor) else type(depth).__name__
            raise ValueError(f"integrate: depth must be [H, W] or [V, H, W], got {got}")
        single = depth.dim() == 2
        if single:
            if isinstance(cameras, (list, tuple)):
                raise ValueError("integrate: a [H, W] depth map takes one camera, not a list")
            cameras = [cameras]
        elif not isinstance(cameras, (list, tuple)) or len(cameras) != depth.shape[0] or len(cameras) < 1:
            n = len(cameras) if isinstance(cameras, (list, tuple)) else type(cameras).__name__
            raise ValueError(f"integrate: a [V, H, W] depth map takes a list of V >= 1 cameras, got {n} for "
                             f"{tuple(depth.shape)}")
        V, (H, W) = len(cameras), depth.shape[-2:]
        if H < 1 or W < 1:
            raise ValueError(f"integrate: the maps must be at least 1x1, got {W}x{H}")
        lead = () if single else (V,)
        depth = self._check_map(depth, "depth", lead + (H, W))
        if alpha is not None:
            alpha = self._check_map(alpha, "alpha", lead + (H, W))
        if image is not None:
            image = self._check_map(image, "image", lead + (3, H, W))
        for cam in cameras:
            if (int(cam._width), int(cam._height)) != (W, H):
                raise ValueError(f"integrate: a camera of {cam._width}x{cam._height} with maps of {W}x{H}")
        if math.isnan(alpha_min) or math.isnan(depth_max):
            raise ValueError(f"integrate: alpha_min and depth_max must not be NaN, got {alpha_min!r}, {depth_max!r}")
        rows = torch.tensor([camera_row(c)[:N.GS_TSDF_CAMERA_FLOATS] for c in cameras], dtype=torch.float32).to(self.device)
        a = N.GsTsdfIntegrateArgs(self._vol(), V, W, H, rows.data_ptr(), depth.data_ptr(), N.ptr(alpha), N.ptr(image),
                                  self.near, self.trunc, float(alpha_min), float(depth_max))
        N.check(N.load().gs_tsdf_integrate(C.byref(a), N.stream_ptr(self.device)), "gs_tsdf_integrate")

    @torch.no_grad()
    def integrate_renders(self, renderer, gaussians, cameras, settings=None, depth: str = "median",
                          views_per_launch: int = 8, **render_kwargs) -> None:
        """Render every camera (renderer.render(camera, gaussians, settings,
        **render_kwargs); settings: a RenderSettings, a callable camera ->
        RenderSettings, or None: the camera's own size on a black background)
        and fuse the depth maps with the renders' alpha and image,
        up to views_per_launch of one size per launch.  depth: "median" takes
        out["median_depth"] of depth_distortion=True, "expected" out["depth"]."""
        if depth not in ("median", "expected"):
            raise ValueError(f"depth must be 'median' or 'expected', got {depth!r}")
        if isinstance(views_per_launch, bool) or not isinstance(views_per_launch, int) or views_per_launch < 1:
            raise ValueError(f"views_per_launch must be an integer >= 1, got {views_per_launch!r}")
        from .renderer import RenderSettings
        if depth == "median":
            render_kwargs = dict(render_kwargs, depth_distortion=True)
        batch: list = []

        def flush():
            if batch:
                cams, d, al, im = zip(*batch)
                self.integrate(torch.stack(d), list(cams), alpha=torch.stack(al), image=torch.stack(im))
                batch.clear()

        for cam in cameras:
            if settings is None:
                st = RenderSettings(cam._height, cam._width, torch.zeros(3))
            else:
                st = settings(cam) if callable(settings) else settings
            out = renderer.render(cam, gaussians, st, **render_kwargs)
            d = out["median_depth"] if depth == "median" else out["depth"]
            hw = tuple(d.shape[-2:])  # (the blend's alpha and depth are [1, H, W])
            if batch and tuple(batch[0][1].shape) != hw:
                flush()
            batch.append((cam, d.float().reshape(hw), out["alpha"].float().reshape(hw), out["image"].float()))
            if len(batch) == views_per_launch:
                flush()
        flush()

    # -- extraction --------------------------------------------------------
    @torch.no_grad()
    def extract_mesh(self, min_weight: float = 1.0) -> Dict[str, Optional[torch.Tensor]]:
        """Surface nets over the cells whose 8 corners all have weight >=
        min_weight: {"vertices" [Vn, 3] fp32, "faces" [Fn, 3] int32, "colors"
        [Vn, 3] fp32 or None without a colour volume}.  One vertex per cell
        the surface crosses, two triangles per crossed node edge that four
        such cells surround, wound so that normals point from inside (tsdf <
        0) to outside; manifold wherever the volume is observed.  One
        classification launch, two prefix sums, one host read of the two
        totals, one emission.  The same volume gives the same bits."""
        if math.isnan(min_weight):
            raise ValueError("min_weight must not be NaN")
        nx, ny, nz = self.dims
        dev = self.device
        empty = {"vertices": torch.zeros((0, 3), dtype=torch.float32, device=dev),
                 "faces": torch.zeros((0, 3), dtype=torch.int32, device=dev),
                 "colors": None if self.color is None else torch.zeros((0, 3), dtype=torch.float32, device=dev)}
        cell_active = torch.empty(((nz - 1) * (ny - 1) * (nx - 1),), dtype=torch.uint8, device=dev)
        node_tris = torch.empty((nz * ny * nx,), dtype=torch.uint8, device=dev)
        node_mask = torch.empty_like(node_tris)
        a = N.GsMeshArgs(self._vol(), float(min_weight), N.ptr(cell_active) if cell_active.numel() else None,
                         node_tris.data_ptr(), node_mask.data_ptr())
        lib, stream = N.load(), N.stream_ptr(dev)
        N.check(lib.gs_mesh_classify(C.byref(a), stream), "gs_mesh_classify")
        if cell_active.numel() == 0:
            return empty
        cell_rank = torch.cumsum(cell_active, 0, dtype=torch.int32)
        # (six triangles a node could pass int32 only from 2^31 / 6 nodes on: then the total is summed wide)
        wide = 6 * node_tris.numel() >= 2 ** 31
        node_faces = torch.cumsum(node_tris, 0, dtype=torch.int32)
        totals = torch.stack([cell_rank[-1].to(torch.int64),
                              node_tris.sum(dtype=torch.int64) if wide else node_faces[-1].to(torch.int64)]).tolist()
        vn, fn = int(totals[0]), int(totals[1])
        if fn >= 2 ** 31:
            raise ValueError(f"the mesh would have {fn} triangles: more than int32 indexes")
        if vn == 0:
            return empty
        vertices = torch.empty((vn, 3), dtype=torch.float32, device=dev)
        colors = None if self.color is None else torch.empty((vn, 3), dtype=torch.float32, device=dev)
        faces = torch.empty((fn, 3), dtype=torch.int32, device=dev)
        a.cell_rank, a.node_faces = cell_rank.data_ptr(), node_faces.data_ptr()
        a.num_vertices, a.num_faces = vn, fn
        a.vertices, a.colors, a.faces = vertices.data_ptr(), N.ptr(colors), N.ptr(faces) if fn else None
        N.check(lib.gs_mesh_emit(C.byref(a), stream), "gs_mesh_emit")
        return {"vertices": vertices, "faces": faces, "colors": colors}


def save_mesh_ply(path, vertices, faces, colors=None) -> None:
    """Write a binary little-endian PLY: float x y z per vertex, with `colors`
    also uchar red green blue (the colours clamped to [0, 1] and rounded), and
    a `list uchar int vertex_indices` per face.  Tensors or arrays."""
    to_np = lambda t: t.detach().cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)
    v, f = to_np(vertices), to_np(faces)
    if v.ndim != 2 or v.shape[1] != 3:
        raise ValueError(f"vertices must be [Vn, 3], got {v.shape}")
    if f.ndim != 2 or f.shape[1] != 3 or f.dtype.kind not in "iu":
        raise ValueError(f"faces must be integer [Fn, 3], got {f.dtype} {f.shape}")
    if f.size and (f.min() < 0 or f.max() >= v.shape[0]):
        raise ValueError(f"faces index vertices outside [0, {v.shape[0]})")
    fields = [("x", "<f4"), ("y", "<f4"), ("z", "<f4")]
    header = ["ply", "format binary_little_endian 1.0", f"element vertex {v.shape[0]}",
              "property float x", "property float y", "property float z"]
    if colors is not None:
        c = to_np(colors)
        if c.shape != v.shape:
            raise ValueError(f"colors must be [Vn, 3] like the vertices, got {c.shape}")
        fields += [("red", "u1"), ("green", "u1"), ("blue", "u1")]
        header += ["property uchar red", "property uchar green", "property uchar blue"]
    header += [f"element face {f.shape[0]}", "property list uchar int vertex_indices", "end_header"]
    vert = np.empty(v.shape[0], dtype=fields)
    vert["x"], vert["y"], vert["z"] = v[:, 0], v[:, 1], v[:, 2]
    if colors is not None:
        c8 = np.rint(np.clip(np.nan_to_num(c.astype(np.float64)), 0.0, 1.0) * 255.0).astype(np.uint8)
        vert["red"], vert["green"], vert["blue"] = c8[:, 0], c8[:, 1], c8[:, 2]
    face = np.empty(f.shape[0], dtype=[("n", "u1"), ("i", "<i4", (3,))])
    face["n"], face["i"] = 3, f
    with open(path, "wb") as fh:
        fh.write(("\n".join(header) + "\n").encode("ascii"))
        fh.write(vert.tobytes())
        fh.write(face.tobytes())


__all__ = ["TSDFVolume", "save_mesh_ply"]
