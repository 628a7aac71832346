"""Yardsticks of the screen-space low-pass filter (gs_screen_filter in
include/gsplat_mi355x.h), test infrastructure:

1. The filtered statement: tests/project_reference.py's projection with
     V = cov2d + s I
   in place of cov2d for the conic, the radius, the cull test and its margin,
   and, when compensating, opacity rho with
     rho = sqrt(max(det cov2d / det V, 2.5e-5)),
   at any floating dtype (fp64: the reference; fp32: the quantile rule's
   yardstick), and its autograd.

2. An equivalent scene for the pinned oracle, which knows no filter.  In exact
   arithmetic V0 + s I is the projection of
     cov3d' = cov3d + Rv^-1 diag(s Z^2 / fx^2, s Z^2 / fy^2, 0) Rv^-T
   since J diag(.) J^T = s I for the perspective Jacobian J at depth Z, and the
   compensation is opacity' = opacity rho.  Both are formed in fp64 from the
   fp32 inputs and rounded once.  (The inverse of Rv, not its transpose: an fp32
   view is orthogonal to 1e-7 only.)  Gradients at the equivalent scene are
   pulled back through the map with autograd in fp64.
"""
from __future__ import annotations

import dataclasses
import math
from typing import Dict

import numpy as np
import torch

import golden_io as G
import project_reference as PR

RHO_FLOOR = 2.5e-5  # Mip-Splatting's floor on det V0 / det V


def _filtered(out: Dict[str, torch.Tensor], cam: PR.Camera, xyz, s: float, compensate: bool):
    """`out` (PR.project's) with cov2d, conics, radii, vis, margin and opacity replaced; also `ratio`."""
    dt = xyz.dtype
    V0 = out["cov2d"]
    V = V0 + s * torch.eye(2, dtype=dt)
    a, b, c, d = V[:, 0, 0], V[:, 0, 1], V[:, 1, 0], V[:, 1, 1]
    det = a * d - b * c
    Q = torch.stack([d / det, -b / det, -c / det, a / det], -1).reshape(-1, 2, 2)
    hm, hd = 0.5 * (a + d), 0.5 * (a - d)
    lmax = hm + torch.sqrt(hd * hd + c * c)
    r = (3.0 * torch.sqrt(lmax)).clamp(cam.radius_min, cam.radius_max)
    mx, my = out["means2d"].unbind(-1)
    Z = out["Z"]
    W, H = float(cam.width), float(cam.height)
    vis = (Z > 0) & (mx >= -r) & (mx < W + r) & (my >= -r) & (my < H + r) & (r > 0)
    view = torch.tensor(cam.view, dtype=dt).reshape(3, 4)
    sx, sy = mx.abs() + r + W, my.abs() + r + H
    sz = (xyz.abs() * view[2, :3].abs()).sum(-1) + view[2, 3].abs()
    margin = torch.stack([(mx + r).abs() / sx, (W + r - mx).abs() / sx, (my + r).abs() / sy,
                          (H + r - my).abs() / sy, Z.abs() / sz], -1).min(-1).values.detach()
    det0 = V0[:, 0, 0] * V0[:, 1, 1] - V0[:, 0, 1] * V0[:, 1, 0]
    ratio = det0 / det
    res = dict(out)
    res.update(cov2d=V, conics=Q, radii=r, vis=vis, margin=margin, ratio=ratio.detach())
    if compensate:
        res["opacity"] = out["opacity"] * torch.sqrt(ratio.clamp_min(RHO_FLOOR))
    return res


def project(cam: PR.Camera, s: float, compensate: bool, xyz, color_logits, opacity, **kw):
    """PR.project with the screen filter (s = 0: PR.project itself, plus `ratio`)."""
    out = PR.project(cam, xyz, color_logits, opacity, **kw)
    return _filtered(out, cam, xyz, float(s), bool(compensate) and s > 0)


def forward(cam, inputs, s, compensate, dtype=torch.float64, sh_degree=0, opacity_is_logit=False):
    with torch.no_grad():
        return project(cam, s, compensate, sh_degree=sh_degree, opacity_is_logit=opacity_is_logit,
                       **PR.cast_inputs(inputs, dtype))


def backward(cam, inputs, s, compensate, acc, g_means2d=None, g_conics=None, dtype=torch.float64, sh_degree=0,
             opacity_is_logit=False):
    """PR.backward of the filtered statement: dL/d(parameter), L as in project_reference's docstring."""
    p = PR.cast_inputs(inputs, dtype, requires_grad=True)
    if sh_degree == 0:
        p.pop("sh_rest", None)
    out = project(cam, s, compensate, sh_degree=sh_degree, opacity_is_logit=opacity_is_logit, **p)
    cot = [None if t is None else t.to(dtype) for t in (acc, g_means2d, g_conics)]
    L = PR.blend_scalar(out, *cot).sum()
    names = list(p)
    grads = torch.autograd.grad(L, [p[k] for k in names], allow_unused=True)
    return {k: (torch.zeros_like(p[k]) if g is None else g) for k, g in zip(names, grads)}


def backward_view(cam, inputs, s, compensate, acc, g_means2d=None, g_conics=None, opacity_is_logit=False):
    """dL/d(view rows [R | t]) [3,4] of the filtered statement in fp64 (sh_degree
    0).  The projection under view [R | t] of (xyz, Sigma) is the projection
    under the identity view of (R xyz + t, R Sigma R^T): the view is a leaf of
    that map, and the filtered statement runs on its outputs."""
    dt = torch.float64
    p = PR.cast_inputs(inputs, dt)
    view = torch.tensor(cam.view, dtype=dt).reshape(3, 4).requires_grad_(True)
    R, t = view[:, :3], view[:, 3]
    S = p["cov3d"].reshape(-1, 3, 3) if "cov3d" in p else PR.covariance(p["scaling"], p["rotation"])
    ident = dataclasses.replace(cam, view=(1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 0.0, 1.0, 0.0))
    out = project(ident, s, compensate, p["xyz"] @ R.T + t, p["color_logits"], p["opacity"], cov3d=R @ S @ R.T,
                  opacity_is_logit=opacity_is_logit)
    cot = [None if x is None else x.to(dt) for x in (acc, g_means2d, g_conics)]
    return torch.autograd.grad(PR.blend_scalar(out, *cot).sum(), view)[0]


# ------------------------------------------------------ equivalent scene ----
def intrinsics(scene):
    """(fx, fy) as the renderer derives them: python double, rounded to fp32."""
    cw = scene.width if scene.cam_width is None else scene.cam_width
    ch = scene.height if scene.cam_height is None else scene.cam_height
    return (float(np.float32(0.5 * cw / math.tan(scene.fovx * 0.5))),
            float(np.float32(0.5 * ch / math.tan(scene.fovy * 0.5))))


def equivalent_map(xyz, cov3d, opacity, wv, fx, fy, s, compensate, use_inverse=True):
    """(cov3d', opacity', ratio) in fp64 torch, differentiable in xyz, cov3d [n,3,3] and opacity [n]."""
    dt = torch.float64
    wv = torch.as_tensor(np.asarray(wv, np.float32)).to(dt)
    Rv, tv = wv[:3, :3], wv[:3, 3]
    Xc = xyz @ Rv.T + tv
    X, Y, Z = Xc.unbind(-1)
    zero = torch.zeros_like(Z)
    D = torch.stack([s * Z * Z / (fx * fx), zero, zero, zero, s * Z * Z / (fy * fy), zero, zero, zero, zero],
                    -1).reshape(-1, 3, 3)
    Ri = torch.linalg.inv(Rv) if use_inverse else Rv.T
    cov_eq = cov3d + Ri @ D @ Ri.T
    J = torch.stack([fx / Z, zero, -fx * X / (Z * Z), zero, -fy / Z, fy * Y / (Z * Z)], -1).reshape(-1, 2, 3)
    V0 = J @ (Rv @ cov3d @ Rv.T) @ J.transpose(1, 2) + 1e-6 * torch.eye(2, dtype=dt)
    V = V0 + s * torch.eye(2, dtype=dt)
    det = lambda M: M[:, 0, 0] * M[:, 1, 1] - M[:, 0, 1] * M[:, 1, 0]
    ratio = det(V0) / det(V)
    op_eq = opacity * torch.sqrt(ratio.clamp_min(RHO_FLOOR)) if (compensate and s > 0) else opacity * 1.0
    return cov_eq, op_eq, ratio


def _leaves(scene):
    t = lambda a, shape: torch.tensor(np.asarray(a, np.float32).reshape(shape), dtype=torch.float64, requires_grad=True)
    n = np.asarray(scene.xyz).shape[0]
    return t(scene.xyz, (n, 3)), t(scene.cov3d, (n, 3, 3)), t(scene.opacity, (n,))


def equivalent_scene(scene, s, compensate):
    """The oracle Scene whose unfiltered render is `scene`'s filtered one; also the fp64 ratio det V0 / det V."""
    fx, fy = intrinsics(scene)
    with torch.no_grad():
        cov_eq, op_eq, ratio = equivalent_map(*_leaves(scene), scene.wv, fx, fy, float(s), compensate)
    eq = dataclasses.replace(scene, cov3d=cov_eq.numpy().astype(np.float32), opacity=op_eq.numpy().astype(np.float32))
    return eq, ratio.numpy()


def pull_back(scene, s, compensate, d_xyz, d_cov3d, d_opacity):
    """Gradients at (xyz, cov3d, opacity) of `scene` from the oracle's at its equivalent scene."""
    fx, fy = intrinsics(scene)
    xyz, cov3d, opacity = _leaves(scene)
    cov_eq, op_eq, _ = equivalent_map(xyz, cov3d, opacity, scene.wv, fx, fy, float(s), compensate)
    n = xyz.shape[0]
    T = lambda a, shape: torch.tensor(np.asarray(a, np.float64).reshape(shape))
    L = (cov_eq * T(d_cov3d, (n, 3, 3))).sum() + (op_eq * T(d_opacity, (n,))).sum() + (xyz * T(d_xyz, (n, 3))).sum()
    gx, gc, go = torch.autograd.grad(L, [xyz, cov3d, opacity])
    return dict(xyz=gx.numpy(), cov3d=gc.numpy(), opacity=go.numpy())


def equivalent_fixture(f, s, compensate):
    """A fixture dict with cov3d / opacity replaced by the equivalent scene's (for helpers that take fixtures)."""
    eq, ratio = equivalent_scene(G.scene_of(f), s, compensate)
    g = dict(f)
    g["cov3d"], g["opacity"] = eq.cov3d, eq.opacity
    return g, eq, ratio


# ------------------------------------------------------------ multi-scale ----
def box_average(img, k):
    c, h, w = img.shape
    return img.reshape(c, h // k, k, w // k, k).mean((2, 4))


def downscaled(scene, k):
    """The same view at 1/k of the resolution (same field of view)."""
    cw = scene.width if scene.cam_width is None else scene.cam_width
    ch = scene.height if scene.cam_height is None else scene.cam_height
    assert scene.width % k == 0 and scene.height % k == 0 and cw % k == 0 and ch % k == 0
    return dataclasses.replace(scene, width=scene.width // k, height=scene.height // k, cam_width=cw // k,
                               cam_height=ch // k)


def rmse(a, b):
    return float(np.sqrt(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))
