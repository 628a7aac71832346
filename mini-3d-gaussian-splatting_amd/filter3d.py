"""Mip-Splatting's 3D smoothing filter (Yu et al. 2024, Sec. 4.1; not in the
reference): the other half of the anti-aliased mode, next to
RenderSettings.screen_filter.

Each Gaussian is convolved in world space with an isotropic Gaussian of
standard deviation f = sqrt(variance) / nu, where nu is the highest sampling
rate (focal / depth, pixels per world unit) any training camera saw it at:
no splat is then thinner than what the training views resolved, and a zoom-in
does not show eroded needles.  Three HIP kernels (include/gsplat_mi355x.h,
"3D smoothing filter"):

  Filter3D.update          gs_filter3d_accumulate: nu over all cameras, one launch
  apply_filter_3d          gs_filter3d_forward / _backward: the per-Gaussian map
                           (scaling, opacity logit, f) -> (scaling', opacity')

GaussianRenderer.render(..., filter_3d=Filter3D) puts the map in front of the
projection; apply_filter_3d is public because it is also how a caller bakes
the filter into a model for export.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Tuple

import torch

from . import _native as N


def check_filter_3d_variance(variance) -> None:
    """ValueError for a 3D filter variance no filter can use (negative, NaN or infinite)."""
    v = float(variance)
    if not (v >= 0.0 and math.isfinite(v)):
        raise ValueError(f"the 3D filter's variance must be finite and >= 0 (px^2), got {variance!r}")


def camera_row(camera) -> list:
    """One row of the rate pass: {view[12], fx, fy, cx, cy, W, H}, the values
    camera_params forms for a render of the camera's own size."""
    from .renderer import _host_f32, _world_view
    W, H = camera._width, camera._height
    fx = 0.5 * W / math.tan(camera._FoVx * 0.5)
    fy = 0.5 * H / math.tan(camera._FoVy * 0.5)
    return _host_f32(_world_view(camera), 16)[:12] + [fx, fy, W * 0.5, H * 0.5, float(W), float(H)]


class Filter3D:
    """The 3D filter of `n` Gaussians on `device`: `max_rate` [n] fp32, the
    highest sampling rate seen (0: seen by no camera), and `values` [n] fp32,
    the filter's standard deviation f in world units (what apply_filter_3d
    takes).  variance is the filter's size in px^2 at the sampling rate
    (Mip-Splatting: 0.2); near and margin decide which camera sees a Gaussian
    (depth > near, inside the image grown by margin on every side)."""

    def __init__(self, n: int, device, variance: float = 0.2, near: float = 0.2, margin: float = 0.15):
        check_filter_3d_variance(variance)
        if not (math.isfinite(near) and near > 0.0):
            raise ValueError(f"near must be finite and > 0, got {near!r}")
        if not (math.isfinite(margin) and margin >= 0.0):
            raise ValueError(f"margin must be finite and >= 0, got {margin!r}")
        if int(n) != n or n < 0:
            raise ValueError(f"n must be an integer >= 0, got {n!r}")
        self.n, self.device = int(n), torch.device(device)
        self.variance, self.near, self.margin = float(variance), float(near), float(margin)
        self.max_rate = torch.zeros(self.n, dtype=torch.float32, device=self.device)
        self.device = self.max_rate.device  # ("cuda" resolved to the current device's index)
        self.values = torch.zeros(self.n, dtype=torch.float32, device=self.device)

    @torch.no_grad()
    def accumulate(self, cameras, xyz: torch.Tensor) -> None:
        """max_rate = max(max_rate, the highest rate among `cameras`), one launch."""
        if xyz.dim() != 2 or tuple(xyz.shape) != (self.n, 3) or xyz.dtype != torch.float32 or xyz.device != self.device:
            raise ValueError(f"xyz must be fp32 [{self.n}, 3] on {self.device}, got {xyz.dtype} {tuple(xyz.shape)} "
                             f"on {xyz.device}")
        rows = [camera_row(c) for c in cameras]
        if not rows or self.n == 0:
            return
        if xyz.stride(1) != 1:
            xyz = xyz.contiguous()
        cams = torch.tensor(rows, dtype=torch.float32).to(self.device)
        a = N.GsFilter3dRateArgs(self.n, xyz.data_ptr(), xyz.stride(0), cams.data_ptr(), len(rows), self.near,
                                 self.margin, self.max_rate.data_ptr())
        N.check(N.load().gs_filter3d_accumulate(C.byref(a), N.stream_ptr(self.device)), "gs_filter3d_accumulate")

    @torch.no_grad()
    def update(self, cameras, xyz: torch.Tensor) -> "Filter3D":
        """Recompute the filter from all of `cameras` (the training views):
        values = sqrt(variance) / max_rate where a camera sees the Gaussian,
        elsewhere the largest value among the seen ones (Mip-Splatting's rule
        for unseen points), 0 everywhere when none is seen.  No host read, and
        deterministic: the same cameras and positions give the same bits (on
        every data-parallel rank, when each passes the full camera list)."""
        self.max_rate.zero_()
        self.accumulate(cameras, xyz)
        if self.n:
            seen = self.max_rate > 0
            v = torch.where(seen, math.sqrt(self.variance) / self.max_rate, torch.zeros_like(self.max_rate))
            self.values = torch.where(seen, v, v.max())
        return self

    def state(self) -> dict:
        return {"max_rate": self.max_rate, "values": self.values}

    def load_state(self, state: dict) -> None:
        for name in ("max_rate", "values"):
            t = state[name]
            if tuple(t.shape) != (self.n,) or t.dtype != torch.float32:
                raise ValueError(f"the 3D filter's {name} must be fp32 [{self.n}], got {t.dtype} {tuple(t.shape)}")
            setattr(self, name, t.to(self.device).contiguous())


def _check_map_inputs(scaling, opacity_logit, filter_values) -> None:
    n = int(filter_values.shape[0]) if filter_values.dim() == 1 else -1
    if n < 0 or tuple(scaling.shape) != (n, 3) or opacity_logit.numel() != n or \
            (opacity_logit.dim() and opacity_logit.shape[0] != n):
        raise ValueError(f"apply_filter_3d needs scaling [N, 3], opacity [N] or [N, 1] and filter values [N], got "
                         f"{tuple(scaling.shape)}, {tuple(opacity_logit.shape)}, {tuple(filter_values.shape)}")
    for name, t in (("scaling", scaling), ("opacity", opacity_logit), ("filter values", filter_values)):
        if t.dtype != torch.float32:
            raise ValueError(f"apply_filter_3d: {name} must be fp32, got {t.dtype}")
        if t.device != scaling.device:
            raise ValueError(f"apply_filter_3d: {name} is on {t.device}, scaling on {scaling.device}")


class _ApplyFilter3D(torch.autograd.Function):
    @staticmethod
    def forward(ctx, scaling, opacity_logit, filter_values):
        n = filter_values.shape[0]
        s, o, f = scaling.contiguous(), opacity_logit.contiguous(), filter_values.contiguous()
        s_out, o_out = torch.empty_like(s), torch.empty_like(o)
        a = N.GsFilter3dArgs(n, s.data_ptr(), o.data_ptr(), f.data_ptr(), s_out.data_ptr(), o_out.data_ptr())
        N.check(N.load().gs_filter3d_forward(C.byref(a), N.stream_ptr(s.device)), "gs_filter3d_forward")
        ctx.save_for_backward(s, o, f)
        return s_out, o_out

    @staticmethod
    def backward(ctx, g_s, g_o):
        s, o, f = ctx.saved_tensors
        g_s, g_o = g_s.contiguous(), g_o.contiguous()
        d_s, d_o = torch.empty_like(s), torch.empty_like(o)
        a = N.GsFilter3dArgs(f.shape[0], s.data_ptr(), o.data_ptr(), f.data_ptr(), None, None, g_s.data_ptr(),
                             g_o.data_ptr(), d_s.data_ptr(), d_o.data_ptr())
        N.check(N.load().gs_filter3d_backward(C.byref(a), N.stream_ptr(s.device)), "gs_filter3d_backward")
        return d_s, d_o, None


def apply_filter_3d(scaling: torch.Tensor, opacity_logit: torch.Tensor,
                    filter_values: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The 3D filter's map: log scales [N, 3], opacity logits [N] or [N, 1] and
    the filter's standard deviations f [N] (Filter3D.values) to
      scaling' = 1/2 log(exp(2 scaling) + f^2)            (log scales again)
      opacity' = sigmoid(logit) sqrt(prod_k exp(2 s_k) / (exp(2 s_k) + f^2))
    (a probability, in the logits' shape): the Gaussian convolved with an
    isotropic one of variance f^2, its peak lowered so that it keeps its
    integral.  Differentiable in scaling and the logits; f carries no gradient.
    All fp32 on one device."""
    _check_map_inputs(scaling, opacity_logit, filter_values)
    return _ApplyFilter3D.apply(scaling, opacity_logit, filter_values.detach())


__all__ = ["Filter3D", "apply_filter_3d", "check_filter_3d_variance"]
