"""Camera-pose refinement on top of the renderer's pose gradient.

GaussianRenderer.render() returns dL/d(world_view_transform) to a view that
requires grad (rasterizer.rasterize, gs_project_backward_pose).  CameraPose
parametrises such a view by a 6-vector twist left-multiplied onto a base
pose, so that any torch optimiser refines it:

    pose = CameraPose(camera)
    opt = torch.optim.Adam(pose.parameters(), lr=1e-3)
    out = renderer.render(pose, gaussians, settings)
"""
from __future__ import annotations

import torch
from torch import nn


def _hat(w: torch.Tensor) -> torch.Tensor:
    z = w.new_zeros(())
    return torch.stack([torch.stack([z, -w[2], w[1]]),
                        torch.stack([w[2], z, -w[0]]),
                        torch.stack([-w[1], w[0], z])])


def se3_exp(xi: torch.Tensor) -> torch.Tensor:
    """exp of the twist xi = (v, w) in se(3) as a 4x4 matrix [[R, V v], [0, 1]]:
    w is the axis-angle rotation (theta = |w|), v the translational part,

        R = I + A [w]x + B [w]x^2,    V = I + B [w]x + C [w]x^2,
        A = sin(theta) / theta,  B = (1 - cos(theta)) / theta^2,
        C = (theta - sin(theta)) / theta^3

    -- torch.linalg.matrix_exp([[ [w]x, v ], [0, 0]]) in closed form.  A, B
    and C are functions of theta^2; below a small angle their power series is
    used (the closed forms cancel there, and sqrt has no gradient at 0), so
    the function and its autograd are smooth through xi = 0."""
    if xi.shape != (6,):
        raise ValueError(f"se3_exp takes a 6-vector (v, w), got shape {tuple(xi.shape)}")
    v, w = xi[:3], xi[3:]
    t = (w * w).sum()  # theta^2
    # series to t^4: the first dropped term is t^5 / 11! (A), below the
    # format's rounding for t under the threshold
    small_t = 1e-2 if xi.dtype == torch.float64 else 0.25
    small = t < small_t
    A_s = 1 - t / 6 * (1 - t / 20 * (1 - t / 42 * (1 - t / 72)))
    B_s = 0.5 * (1 - t / 12 * (1 - t / 30 * (1 - t / 56 * (1 - t / 90))))
    C_s = 1.0 / 6 * (1 - t / 20 * (1 - t / 42 * (1 - t / 72 * (1 - t / 110))))
    ts = torch.where(small, torch.ones_like(t), t)  # (the unused branch stays finite, and so does its gradient)
    th = ts.sqrt()
    A_c = th.sin() / th
    B_c = (1 - th.cos()) / ts
    C_c = (th - th.sin()) / (ts * th)
    A, B, C = torch.where(small, A_s, A_c), torch.where(small, B_s, B_c), torch.where(small, C_s, C_c)
    K = _hat(w)
    K2 = K @ K
    eye = torch.eye(3, dtype=xi.dtype, device=xi.device)
    R = eye + A * K + B * K2
    V = eye + B * K + C * K2
    top = torch.cat([R, (V @ v).unsqueeze(1)], 1)
    bottom = torch.cat([xi.new_zeros(3), xi.new_ones(1)]).unsqueeze(0)
    return torch.cat([top, bottom], 0)


class CameraPose(nn.Module):
    """A camera the renderer accepts whose pose is optimised: wraps `camera`
    (anything with _width / _height / _FoVx / _FoVy and world_view_transform,
    method or tensor) and exposes

        world_view_transform() = se3_exp(xi) @ base

    with `xi` a 6-vector parameter (v, w), zero at construction, and `base`
    the wrapped camera's world-to-camera matrix at construction.  The twist
    acts in the camera's frame: w turns the camera about its own axes, v moves
    it along them."""

    def __init__(self, camera, dtype=torch.float32):
        super().__init__()
        self.camera = camera
        wv = camera.world_view_transform
        if callable(wv):
            wv = wv()
        base = torch.as_tensor(wv).detach().to("cpu", dtype).clone()
        if base.shape != (4, 4):
            raise ValueError(f"world_view_transform must be 4x4, got {tuple(base.shape)}")
        self.register_buffer("base", base)
        self.xi = nn.Parameter(torch.zeros(6, dtype=dtype))

    _width = property(lambda self: self.camera._width)
    _height = property(lambda self: self.camera._height)
    _FoVx = property(lambda self: self.camera._FoVx)
    _FoVy = property(lambda self: self.camera._FoVy)

    def world_view_transform(self) -> torch.Tensor:
        return se3_exp(self.xi) @ self.base

    @torch.no_grad()
    def bake(self) -> None:
        """Fold the current twist into the base pose and reset xi to zero."""
        self.base.copy_(se3_exp(self.xi) @ self.base)
        self.xi.zero_()
