"""Normal consistency (2DGS, Huang et al. 2024, Sec. 5; also gsplat and
RaDe-GS; not in the reference): the other half of the geometry regularisation,
next to the depth distortion.  Each Gaussian's normal, composited per pixel
with the colour pass's weights, should agree with the normal of the surface
the depth map implies.  Four HIP kernels (include/gsplat_mi355x.h, "Normal
consistency"):

  gaussian_normals      gs_gaussian_normals_forward / _backward: the camera-space
                        normal of every Gaussian (its shortest axis, facing the
                        camera) from the raw rotation and scaling
  normal_consistency    gs_normal_consistency_forward / _backward: per pixel,
                        1 - alpha (N_r . n_d) with n_d the depth map's normal

The blend between the two is the feature pass: GaussianRenderer.render(...,
normals=True) returns "normals" = sum_i c_i n_i, and
  normal_consistency(out["normals"], out["depth"], out["alpha"], camera).mean()
is 2DGS's normal loss (TrainingConfig.lambda_normal).  There is no CPU path.
"""
from __future__ import annotations

import ctypes as C
import math

import torch

from . import _native as N


class _GaussianNormals(torch.autograd.Function):
    @staticmethod
    def forward(ctx, rotation, scaling, xyz, view):
        n = rotation.shape[0]
        q, s = rotation.contiguous(), scaling.contiguous()
        p = xyz if xyz.stride(1) == 1 and xyz.stride(0) >= 3 else xyz.contiguous()
        out = torch.empty((n, 3), dtype=torch.float32, device=q.device)
        a = N.GsGaussianNormalsArgs(n, q.data_ptr(), s.data_ptr(), p.data_ptr(), p.stride(0),
                                    (C.c_float * 12)(*view), out.data_ptr())
        N.check(N.load().gs_gaussian_normals_forward(C.byref(a), N.stream_ptr(q.device)),
                "gs_gaussian_normals_forward")
        ctx.save_for_backward(q, s, p)
        ctx.view = view
        return out

    @staticmethod
    def backward(ctx, g):
        q, s, p = ctx.saved_tensors
        if not ctx.needs_input_grad[0]:
            return None, None, None, None
        g = g.contiguous()
        d_q = torch.empty_like(q)
        a = N.GsGaussianNormalsArgs(q.shape[0], q.data_ptr(), s.data_ptr(), p.data_ptr(), p.stride(0),
                                    (C.c_float * 12)(*ctx.view), None, g.data_ptr(), d_q.data_ptr())
        N.check(N.load().gs_gaussian_normals_backward(C.byref(a), N.stream_ptr(q.device)),
                "gs_gaussian_normals_backward")
        return d_q, None, None, None


def gaussian_normals(rotation: torch.Tensor, scaling: torch.Tensor, xyz: torch.Tensor, world_view) -> torch.Tensor:
    """The camera-space normal [N, 3] of every Gaussian: the axis of its
    smallest scale (the first among equals) -- column k of R(q / max(|q|,
    1e-12)) -- rotated by the view and turned to face the camera
    (n . (Rv xyz + t) <= 0).  rotation [N, 4] raw (w, x, y, z), scaling [N, 3]
    log and xyz [N, 3], fp32 on one device (the model's _rotation, _scaling,
    _xyz); world_view the 4x4 (or 3x4) world-to-camera matrix, read as host
    scalars as camera_params reads it.  The gradient reaches the rotation only:
    the axis choice and the flip are piecewise constant, and the view is a
    constant here even when it requires grad.  Anything else is a ValueError
    before any launch."""
    n = int(rotation.shape[0]) if isinstance(rotation, torch.Tensor) and rotation.dim() == 2 else -1
    for name, t, cols in (("rotation", rotation, 4), ("scaling", scaling, 3), ("xyz", xyz, 3)):
        if not isinstance(t, torch.Tensor) or t.dim() != 2 or tuple(t.shape) != (n, cols):
            shape = tuple(t.shape) if isinstance(t, torch.Tensor) else type(t).__name__
            raise ValueError(f"gaussian_normals needs rotation [N, 4], scaling [N, 3] and xyz [N, 3]; {name} is {shape}")
        if t.dtype != torch.float32:
            raise ValueError(f"gaussian_normals: {name} must be fp32, got {t.dtype}")
        if t.device != rotation.device:
            raise ValueError(f"gaussian_normals: {name} is on {t.device}, rotation on {rotation.device}")
    from .renderer import _host_f32
    wv = torch.as_tensor(world_view)
    if wv.numel() not in (12, 16):
        raise ValueError(f"gaussian_normals: world_view must be a 4x4 or 3x4 matrix, got {tuple(wv.shape)}")
    view = _host_f32(wv, wv.numel())[:12]
    return _GaussianNormals.apply(rotation, scaling.detach(), xyz.detach(), view)


def camera_intrinsics(camera) -> tuple:
    """(fx, fy, cx, cy) as camera_params forms them."""
    W, H = camera._width, camera._height
    return (0.5 * W / math.tan(camera._FoVx * 0.5), 0.5 * H / math.tan(camera._FoVy * 0.5), W * 0.5, H * 0.5)


class _NormalConsistency(torch.autograd.Function):
    @staticmethod
    def forward(ctx, normals, depth, alpha, intrinsics, want_surface: bool):
        _, H, W = normals.shape
        error = torch.empty((H, W), dtype=torch.float32, device=normals.device)
        surface = torch.empty_like(normals) if want_surface else None
        a = N.GsNormalConsistencyArgs(W, H, *intrinsics, normals.data_ptr(), depth.data_ptr(), alpha.data_ptr(),
                                      error.data_ptr(), N.ptr(surface))
        N.check(N.load().gs_normal_consistency_forward(C.byref(a), N.stream_ptr(normals.device)),
                "gs_normal_consistency_forward")
        ctx.save_for_backward(normals, depth, alpha)
        ctx.intrinsics = intrinsics
        if not want_surface:
            return error
        ctx.mark_non_differentiable(surface)
        return error, surface

    @staticmethod
    def backward(ctx, g_error, *_g_surface):
        normals, depth, alpha = ctx.saved_tensors
        if g_error is None or not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None, None, None
        _, H, W = normals.shape
        g_error = g_error.contiguous()
        d_normals, d_depth = torch.empty_like(normals), torch.empty_like(depth)
        a = N.GsNormalConsistencyArgs(W, H, *ctx.intrinsics, normals.data_ptr(), depth.data_ptr(), alpha.data_ptr(),
                                      None, None, g_error.data_ptr(), d_normals.data_ptr(), d_depth.data_ptr())
        N.check(N.load().gs_normal_consistency_backward(C.byref(a), N.stream_ptr(normals.device)),
                "gs_normal_consistency_backward")
        return (d_normals if ctx.needs_input_grad[0] else None, d_depth if ctx.needs_input_grad[1] else None,
                None, None, None)


def normal_consistency(normals: torch.Tensor, depth: torch.Tensor, alpha: torch.Tensor, camera,
                       return_surface: bool = False):
    """The per-pixel normal consistency error [H, W] of a render:
      error = 1 - alpha (normals . n_d)
    with normals [3, H, W] the rendered sum_i c_i n_i (out["normals"]), and n_d
    the unit normal of the depth map [H, W] (out["depth"]): the cross product
    of the central differences of the back-projected points D r, r = ((x - cx)
    / fx, -(y - cy) / fy, 1), facing the camera; 0 on the one-pixel border and
    where the cross product vanishes, so the error there is exactly 1.  fx, fy,
    cx, cy are the camera's, as camera_params forms them.  Its mean is 2DGS's
    normal loss.  Gradients go to normals and depth; alpha [H, W]
    (out["alpha"]) is a weight and receives none.  return_surface=True returns
    (error, n_d [3, H, W]), the latter detached.  fp32 tensors on a HIP device:
    there is no CPU path."""
    for name, t in (("normals", normals), ("depth", depth), ("alpha", alpha)):
        if not isinstance(t, torch.Tensor) or not t.is_floating_point():
            raise ValueError(f"normal_consistency: {name} must be a floating-point tensor")
    if normals.dim() != 3 or normals.shape[0] != 3:
        raise ValueError(f"normal_consistency: normals must be [3, H, W], got {tuple(normals.shape)}")
    H, W = int(normals.shape[1]), int(normals.shape[2])
    if H < 1 or W < 1:
        raise ValueError(f"normal_consistency: the image must be at least 1x1, got {W}x{H}")
    for name, t in (("depth", depth), ("alpha", alpha)):
        if tuple(t.shape) not in ((H, W), (1, H, W)):
            raise ValueError(f"normal_consistency: {name} must be [{H}, {W}], got {tuple(t.shape)}")
        if t.device != normals.device:
            raise ValueError(f"normal_consistency: {name} is on {t.device}, normals on {normals.device}")
    if not normals.is_cuda:
        raise RuntimeError("normal_consistency needs tensors on a HIP device; there is no CPU path")
    intr = tuple(float(v) for v in camera_intrinsics(camera))
    if not all(math.isfinite(v) for v in intr) or intr[0] == 0.0 or intr[1] == 0.0:
        raise ValueError(f"normal_consistency: the camera's (fx, fy, cx, cy) = {intr} must be finite, fx and fy not 0")
    out = _NormalConsistency.apply(normals.float().contiguous(), depth.float().reshape(H, W).contiguous(),
                                   alpha.detach().float().reshape(H, W).contiguous(), intr, bool(return_surface))
    return out


__all__ = ["gaussian_normals", "normal_consistency"]
