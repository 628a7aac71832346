"""Bilateral-grid appearance compensation (Wang et al., "Bilateral Guided
Radiance Field Processing", SIGGRAPH 2024; HDRNet's slicing; gsplat's
use_bilateral_grid; not in the reference).  Real captures change exposure and
white balance from frame to frame; with nothing to absorb the change the
optimiser explains it with view-dependent colour and floaters.  Each training
image gets a small learnable grid of affine colour transforms, sliced per
pixel -- by position and by the pixel's own gray level -- and applied to the
render before the photometric loss; a total-variation term keeps it smooth.
Three HIP entry points (include/gsplat_mi355x.h, "Bilateral grid"):

  slice_bilateral_grid   gs_bilagrid_slice_forward / _backward: the corrected
                         image, and the gradients to the image and the grid
  bilateral_grid_tv      gs_bilagrid_tv: the total variation and its gradient

BilateralGrids holds one grid per training image with their own FusedAdam
(TrainingConfig.bilateral_grid).  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable

import torch

from . import _native as N
from .optim import FusedAdam

DEFAULT_SHAPE = (16, 16, 8)  # (Gw, Gh, L)


def check_grid_shape(grid_shape, what: str = "grid_shape") -> tuple:
    """(Gw, Gh, L) as integers, or ValueError: each >= 2, Gw and Gh <= 64, L <= 16."""
    ok = isinstance(grid_shape, (tuple, list)) and len(grid_shape) == 3 and \
        all(isinstance(v, int) and not isinstance(v, bool) for v in grid_shape)
    if ok:
        gw, gh, gl = grid_shape
        ok = 2 <= gw <= N.GS_BILAGRID_MAX_XY and 2 <= gh <= N.GS_BILAGRID_MAX_XY and 2 <= gl <= N.GS_BILAGRID_MAX_L
    if not ok:
        raise ValueError(f"{what} must be (Gw, Gh, L) integers with 2 <= Gw, Gh <= {N.GS_BILAGRID_MAX_XY} and "
                         f"2 <= L <= {N.GS_BILAGRID_MAX_L}, got {grid_shape!r}")
    return tuple(grid_shape)


def _slice_args(grid, image, **ptrs):
    _, L, Gh, Gw = grid.shape
    _, H, W = image.shape
    return N.GsBilagridSliceArgs(width=W, height=H, grid_w=Gw, grid_h=Gh, grid_l=L, grid=grid.data_ptr(),
                                 rgb=image.data_ptr(), **ptrs)


class _Slice(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid, image):
        out = torch.empty_like(image)
        a = _slice_args(grid, image, out=out.data_ptr())
        N.check(N.load().gs_bilagrid_slice_forward(C.byref(a), N.stream_ptr(image.device)), "gs_bilagrid_slice_forward")
        ctx.save_for_backward(grid, image)
        return out

    @staticmethod
    def backward(ctx, g_out):
        grid, image = ctx.saved_tensors
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None
        g_out = g_out.contiguous()
        d_grid, d_rgb = torch.empty_like(grid), torch.empty_like(image)
        a = _slice_args(grid, image, g_out=g_out.data_ptr(), d_rgb=d_rgb.data_ptr(), d_grid=d_grid.data_ptr())
        N.check(N.load().gs_bilagrid_slice_backward(C.byref(a), N.stream_ptr(image.device)),
                "gs_bilagrid_slice_backward")
        return (d_grid if ctx.needs_input_grad[0] else None, d_rgb if ctx.needs_input_grad[1] else None)


class _Tv(torch.autograd.Function):
    @staticmethod
    def forward(ctx, grid):
        _, L, Gh, Gw = grid.shape
        tv = torch.empty((), dtype=torch.float32, device=grid.device)
        d_grid = torch.empty_like(grid)
        a = N.GsBilagridTvArgs(Gw, Gh, L, grid.data_ptr(), tv.data_ptr(), d_grid.data_ptr())
        N.check(N.load().gs_bilagrid_tv(C.byref(a), N.stream_ptr(grid.device)), "gs_bilagrid_tv")
        ctx.save_for_backward(d_grid)  # (closed form: the one launch made it)
        return tv

    @staticmethod
    def backward(ctx, g):
        (d_grid,) = ctx.saved_tensors
        return g * d_grid


def _check_grid(grid, what: str) -> None:
    if not isinstance(grid, torch.Tensor) or grid.dim() != 4 or grid.shape[0] != N.GS_BILAGRID_CHANNELS:
        shape = tuple(grid.shape) if isinstance(grid, torch.Tensor) else type(grid).__name__
        raise ValueError(f"{what}: grid must be [12, L, Gh, Gw], got {shape}")
    if grid.dtype != torch.float32:
        raise ValueError(f"{what}: grid must be fp32, got {grid.dtype}")
    check_grid_shape((int(grid.shape[3]), int(grid.shape[2]), int(grid.shape[1])), f"{what}: the grid's shape")


def slice_bilateral_grid(grid: torch.Tensor, image: torch.Tensor) -> torch.Tensor:
    """The image [3, H, W] corrected by the grid [12, L, Gh, Gw] (channel 4c + k
    entry (c, k) of a 3x4 affine matrix): at pixel (x, y) the grid is sliced
    trilinearly at u = (x + 0.5) / W (Gw - 1), v = (y + 0.5) / H (Gh - 1) and
    z = clamp(0.299 r + 0.587 g + 0.114 b, 0, 1) (L - 1) -- torch's 5-D
    grid_sample, bilinear, border padding, align_corners -- and
    out[c] = A[c,0] r + A[c,1] g + A[c,2] b + A[c,3].  The identity grid returns
    the image bit for bit.  Gradients go to both: to the image through the
    affine map and, where 0 < gray < 1, through z; the grid's gradient is the
    same bits every run.  fp32 tensors on one HIP device: there is no CPU
    path."""
    what = "slice_bilateral_grid"
    _check_grid(grid, what)
    if not isinstance(image, torch.Tensor) or image.dim() != 3 or image.shape[0] != 3:
        shape = tuple(image.shape) if isinstance(image, torch.Tensor) else type(image).__name__
        raise ValueError(f"{what}: image must be [3, H, W], got {shape}")
    if image.dtype != torch.float32:
        raise ValueError(f"{what}: image must be fp32, got {image.dtype}")
    if image.shape[1] < 1 or image.shape[2] < 1:
        raise ValueError(f"{what}: the image must be at least 1x1, got {image.shape[2]}x{image.shape[1]}")
    if image.device != grid.device:
        raise ValueError(f"{what}: image is on {image.device}, grid on {grid.device}")
    if not grid.is_cuda:
        raise RuntimeError(f"{what} needs tensors on a HIP device; there is no CPU path")
    return _Slice.apply(grid.contiguous(), image.contiguous())


def bilateral_grid_tv(grid: torch.Tensor) -> torch.Tensor:
    """The total variation of one grid, a scalar: the mean squared difference
    of neighbouring nodes along x, plus that along y, plus that along z, each
    mean over its axis' own pairs and all 12 channels.  The kernel writes the
    value and its (closed-form) gradient in one launch; the backward scales
    the latter."""
    _check_grid(grid, "bilateral_grid_tv")
    if not grid.is_cuda:
        raise RuntimeError("bilateral_grid_tv needs a tensor on a HIP device; there is no CPU path")
    return _Tv.apply(grid.contiguous())


def identity_grid(grid_shape=DEFAULT_SHAPE, device=None) -> torch.Tensor:
    """[12, L, Gh, Gw] with [I | 0] at every node."""
    gw, gh, gl = check_grid_shape(grid_shape)
    g = torch.zeros((N.GS_BILAGRID_CHANNELS, gl, gh, gw), dtype=torch.float32, device=device)
    g[0] = g[5] = g[10] = 1.0
    return g


class BilateralGrids:
    """One bilateral grid per training image: num_images leaf parameters
    [12, L, Gh, Gw], each the identity transform at every node, and their own
    FusedAdam (eps 1e-15).  That optimizer skips parameters without a gradient
    and counts steps per parameter, so a step updates the grids that took part
    in it and leaves every other image's grid and moments bit for bit."""

    def __init__(self, num_images: int, device, grid_shape=DEFAULT_SHAPE, lr: float = 2e-3):
        if isinstance(num_images, bool) or not isinstance(num_images, int) or num_images < 1:
            raise ValueError(f"BilateralGrids needs num_images >= 1, got {num_images!r}")
        self.grid_shape = check_grid_shape(grid_shape)
        device = torch.device(device)
        self.grids = [identity_grid(self.grid_shape, device).requires_grad_(True) for _ in range(num_images)]
        self.optimizer = FusedAdam(self.grids, lr=lr, eps=1e-15)

    def __len__(self) -> int:
        return len(self.grids)

    def _index(self, index) -> int:
        if isinstance(index, bool) or not isinstance(index, int) or not 0 <= index < len(self.grids):
            raise ValueError(f"grid index must be an integer in [0, {len(self.grids)}), got {index!r}")
        return index

    def slice(self, index: int, image: torch.Tensor) -> torch.Tensor:
        """slice_bilateral_grid with image `index`'s grid."""
        return slice_bilateral_grid(self.grids[self._index(index)], image)

    def tv(self, index: int) -> torch.Tensor:
        return bilateral_grid_tv(self.grids[self._index(index)])

    def zero_grad(self) -> None:
        self.optimizer.zero_grad()

    def set_lr(self, lr: float) -> None:
        for group in self.optimizer.param_groups:
            group["lr"] = lr

    def set_grads(self, grads: Dict[int, torch.Tensor]) -> None:
        """Replace the gradients: image index -> [12, L, Gh, Gw]; every other grid has none."""
        self.zero_grad()
        for index, g in grads.items():
            self.grids[self._index(index)].grad = g

    def step(self) -> None:
        """One Adam step of the grids that have a gradient."""
        self.optimizer.step()

    # -- checkpoints -------------------------------------------------------
    def state(self) -> Dict[str, torch.Tensor]:
        """grids, both moments [num_images, 12, L, Gh, Gw] and the per-image
        step counts [num_images] int64 (0 and zero moments for an image no
        step has updated)."""
        st = [self.optimizer.state.get(p, {}) for p in self.grids]
        zeros = torch.zeros_like(self.grids[0])
        return {"grids": torch.stack([p.detach() for p in self.grids]),
                "m": torch.stack([s.get("exp_avg", zeros) for s in st]),
                "v": torch.stack([s.get("exp_avg_sq", zeros) for s in st]),
                "step": torch.tensor([int(s.get("step", 0)) for s in st], dtype=torch.int64)}

    def load_state(self, state: Dict[str, torch.Tensor]) -> None:
        want = (len(self.grids),) + tuple(self.grids[0].shape)
        for name in ("grids", "m", "v"):
            t = state[name]
            if tuple(t.shape) != want or t.dtype != torch.float32:
                raise ValueError(f"bilateral grid state {name!r} must be fp32 {want}, got {t.dtype} {tuple(t.shape)}")
        steps = state["step"]
        if tuple(steps.shape) != (len(self.grids),):
            raise ValueError(f"bilateral grid state 'step' must be [{len(self.grids)}], got {tuple(steps.shape)}")
        dev = self.grids[0].device
        with torch.no_grad():
            for i, p in enumerate(self.grids):
                p.copy_(state["grids"][i])
                self.optimizer.state.pop(p, None)
                if int(steps[i]) > 0:
                    self.optimizer.state[p] = {"step": int(steps[i]),
                                               "exp_avg": state["m"][i].to(dev).clone().contiguous(),
                                               "exp_avg_sq": state["v"][i].to(dev).clone().contiguous()}
        self.zero_grad()

    def parameters(self) -> Iterable[torch.Tensor]:
        return list(self.grids)


__all__ = ["slice_bilateral_grid", "bilateral_grid_tv", "identity_grid", "BilateralGrids", "check_grid_shape"]
