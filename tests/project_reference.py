"""Plain torch statement of the projection stage (k_project_fwd) and, through
autograd, of its backward (k_project_bwd), at any floating dtype (test
infrastructure; fp64 is the reference, fp32 the yardstick).

Written from include/gsplat_mi355x.h (gs_camera, gs_gaussians, gs_project_args,
gs_project_bwd_args) and the kernel's comments:

  Sigma  = R(q) diag(exp(s)^2) R(q)^T, q normalised twice (floor 1e-12), or the
           given cov3d
  Xc     = Rv Xw + Tv                              (X, Y, Z)
  mean   = (fx X / Z + cx, -fy Y / Z + cy)
  J      = [[fx/Z, 0, -fx X/Z^2], [0, -fy/Z, fy Y/Z^2]]
  cov2d  = J (Rv Sigma Rv^T) J^T + 1e-6 I
  Q      = inv(cov2d), the full 2x2 inverse (cov2d is not symmetrised)
  lmax   = (a + d)/2 + sqrt(((a - d)/2)^2 + c^2), c = cov2d[1][0] (lower triangle)
  radius = clamp(3 sqrt(lmax), radius_min, radius_max)
  vis    = Z > 0 and -r <= mx < W + r and -r <= my < H + r and r > 0
  colour = sigmoid(DC logits + SH terms of degree 1..sh_degree)
  opacity as given, or sigmoid(opacity) when it is the model's logit

The backward is autograd of the scalar (acc = one row of grad_sums,
GS_PAIR_GRAD_FLOATS = 10, summed over the Gaussians)
  L = <acc[0:2], mean> + acc[2] Q00 + acc[3] (Q01 + Q10) + acc[4] Q11
      + acc[5] opacity + <acc[6:9], colour> + acc[9] Z
      (+ <g_means2d, mean> + <g_conics, Q> when those cotangents are given)
for every Gaussian, visible or not: the kernel's backward has no visibility
test of its own (a culled Gaussian's acc is zero in a frame)."""
from __future__ import annotations

import math
from dataclasses import dataclass
from typing import Dict, Optional, Tuple

import numpy as np
import torch

from sh_reference import sh_logits


def _f32(x) -> float:
    return float(np.float32(x))


@dataclass
class Camera:
    """gs_camera's scalars, each already rounded to fp32 (the kernel's values)."""
    width: int
    height: int
    fx: float
    fy: float
    cx: float
    cy: float
    view: Tuple[float, ...]  # 12 floats: rows [R | t]
    radius_min: float = _f32(0.01)
    radius_max: float = 50.0
    tile_size: int = 16

    @property
    def campos(self) -> Tuple[float, float, float]:
        """-R^T t in double from the fp32 view, rounded to fp32 (gs_camera.campos)."""
        v = self.view
        R = ((v[0], v[1], v[2]), (v[4], v[5], v[6]), (v[8], v[9], v[10]))
        t = (v[3], v[7], v[11])
        return tuple(_f32(-(R[0][j] * t[0] + R[1][j] * t[1] + R[2][j] * t[2])) for j in range(3))


def make_camera(width, height, fovx, fovy, wv=None, radius_min=0.01, radius_max=50.0, tile_size=16,
                cam_width=None, cam_height=None) -> Camera:
    """Intrinsics as the renderer derives them (python double, rounded to fp32)."""
    cw, ch = (width if cam_width is None else cam_width), (height if cam_height is None else cam_height)
    wv = np.eye(4) if wv is None else np.asarray(wv, np.float64)
    view = tuple(_f32(x) for x in np.asarray(wv)[:3, :].reshape(-1))
    return Camera(int(width), int(height), _f32(0.5 * cw / math.tan(fovx * 0.5)), _f32(0.5 * ch / math.tan(fovy * 0.5)),
                  _f32(cw * 0.5), _f32(ch * 0.5), view, _f32(radius_min), _f32(radius_max), int(tile_size))


def covariance(scaling: torch.Tensor, rotation: torch.Tensor) -> torch.Tensor:
    """[n,3] log-sigma, [n,4] q = (w, x, y, z) -> [n,3,3]."""
    q = rotation
    for _ in range(2):  # get_rotation normalises, build_rotation_matrix again
        q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12)
    w, x, y, z = q.unbind(-1)
    R = torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                     2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                     2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(-1, 3, 3)
    s2 = torch.exp(scaling) ** 2
    return (R * s2[:, None, :]) @ R.transpose(1, 2)


def project(cam: Camera, xyz, color_logits, opacity, scaling=None, rotation=None, cov3d=None, sh_rest=None,
            sh_degree: int = 0, opacity_is_logit: bool = False) -> Dict[str, torch.Tensor]:
    """The forward, in the dtype of xyz.  Returns means2d [n,2], cov2d and
    conics [n,2,2], radii, vis, colour [n,3], opacity [n], Z [n] and margin
    [n]: the smallest relative distance of a cull comparison to its boundary."""
    dt = xyz.dtype
    S = cov3d.reshape(-1, 3, 3) if cov3d is not None else covariance(scaling, rotation)
    V = torch.tensor(cam.view, dtype=dt).reshape(3, 4)
    Rv, tv = V[:, :3], V[:, 3]
    Xc = xyz @ Rv.T + tv
    X, Y, Z = Xc.unbind(-1)
    mx = cam.fx * X / Z + cam.cx
    my = -cam.fy * Y / Z + cam.cy
    C = Rv @ S @ Rv.T
    zero = torch.zeros_like(Z)
    J = torch.stack([cam.fx / Z, zero, -cam.fx * X / (Z * Z), zero, -cam.fy / Z, cam.fy * Y / (Z * Z)], -1).reshape(-1, 2, 3)
    cov2d = J @ C @ J.transpose(1, 2) + 1e-6 * torch.eye(2, dtype=dt)
    a, b, c, d = cov2d[:, 0, 0], cov2d[:, 0, 1], cov2d[:, 1, 0], cov2d[:, 1, 1]
    det = a * d - b * c
    Q = torch.stack([d / det, -b / det, -c / det, a / det], -1).reshape(-1, 2, 2)
    hm, hd = 0.5 * (a + d), 0.5 * (a - d)
    lmax = hm + torch.sqrt(hd * hd + c * c)
    r = (3.0 * torch.sqrt(lmax)).clamp(cam.radius_min, cam.radius_max)
    W, H = float(cam.width), float(cam.height)
    vis = (Z > 0) & (mx >= -r) & (mx < W + r) & (my >= -r) & (my < H + r) & (r > 0)
    # each comparison's distance to its boundary, relative to its operands' size
    sx, sy = mx.abs() + r + W, my.abs() + r + H
    sz = (xyz.abs() * Rv[2].abs()).sum(-1) + tv[2].abs()
    margin = torch.stack([(mx + r).abs() / sx, (W + r - mx).abs() / sx, (my + r).abs() / sy,
                          (H + r - my).abs() / sy, Z.abs() / sz], -1).min(-1).values.detach()
    logits = color_logits
    if sh_degree > 0:
        logits = sh_logits(xyz, color_logits, sh_rest.reshape(-1, 15, 3), torch.tensor(cam.campos, dtype=dt), sh_degree)
    op = torch.sigmoid(opacity) if opacity_is_logit else opacity
    return dict(means2d=torch.stack([mx, my], -1), cov2d=cov2d, conics=Q, radii=r, vis=vis,
                color=torch.sigmoid(logits), opacity=op, Z=Z, margin=margin)


def blend_scalar(out: Dict[str, torch.Tensor], acc, g_means2d=None, g_conics=None) -> torch.Tensor:
    """Per-Gaussian [n] terms of L (module docstring); L is their sum."""
    Q = out["conics"]
    L = (acc[:, 0:2] * out["means2d"]).sum(-1) + acc[:, 2] * Q[:, 0, 0] + acc[:, 3] * (Q[:, 0, 1] + Q[:, 1, 0]) + \
        acc[:, 4] * Q[:, 1, 1] + acc[:, 5] * out["opacity"] + (acc[:, 6:9] * out["color"]).sum(-1) + acc[:, 9] * out["Z"]
    if g_means2d is not None:
        L = L + (g_means2d * out["means2d"]).sum(-1)
    if g_conics is not None:
        L = L + (g_conics.reshape(-1, 2, 2) * Q).sum((-1, -2))
    return L


PARAMS = ("xyz", "color_logits", "opacity", "scaling", "rotation", "cov3d", "sh_rest")


def cast_inputs(inputs: Dict[str, Optional[torch.Tensor]], dtype, requires_grad=False) -> Dict[str, torch.Tensor]:
    """The fp32 parameter tensors of `inputs` (PARAMS; missing / None: absent) in `dtype`, as fresh leaves."""
    out = {}
    for k in PARAMS:
        t = inputs.get(k)
        if t is not None:
            out[k] = t.detach().to(dtype).clone().requires_grad_(requires_grad)
    return out


def forward(cam: Camera, inputs, dtype=torch.float64, sh_degree=0, opacity_is_logit=False):
    with torch.no_grad():
        return project(cam, sh_degree=sh_degree, opacity_is_logit=opacity_is_logit, **cast_inputs(inputs, dtype))


def backward(cam: Camera, inputs, acc, g_means2d=None, g_conics=None, dtype=torch.float64, sh_degree=0,
             opacity_is_logit=False) -> Dict[str, torch.Tensor]:
    """dL/d(parameter) for each parameter present in `inputs` (fp32 tensors,
    cast to `dtype` exactly); acc [n,10], g_means2d [n,2], g_conics [n,4]."""
    p = cast_inputs(inputs, dtype, requires_grad=True)
    if sh_degree == 0:
        p.pop("sh_rest", None)
    out = project(cam, sh_degree=sh_degree, opacity_is_logit=opacity_is_logit, **p)
    cot = [None if t is None else t.to(dtype) for t in (acc, g_means2d, g_conics)]
    L = blend_scalar(out, *cot).sum()
    names = list(p)
    grads = torch.autograd.grad(L, [p[k] for k in names], allow_unused=True)
    return {k: (torch.zeros_like(p[k]) if g is None else g) for k, g in zip(names, grads)}
