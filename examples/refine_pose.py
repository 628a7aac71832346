"""Camera-pose refinement: render a target at the true pose, start from a
perturbed pose, and run Adam on the 6-vector twist of pose.CameraPose.

The renderer returns dL/d(world_view_transform) to a view that requires grad
(gs_project_backward_pose: the projection backward plus a deterministic
reduction over the Gaussians), so the pose is optimised like any tensor:

    pose = CameraPose(camera)                      # xi = 0: the camera's own pose
    opt = torch.optim.Adam(pose.parameters(), lr=2e-3)
    loss = ((renderer.render(pose, gaussians, settings)["image"] - target) ** 2).mean()
    loss.backward(); opt.step()

    python examples/refine_pose.py [--iters 200] [--gaussians 2000] [--size 128]

Prints the loss and the pose error every 20 iterations.  Needs a HIP device
(the renderer has no CPU path).
"""
from __future__ import annotations

import argparse
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _package():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.load_package()


class _Cam:
    """camera._width/_height/_FoVx/_FoVy and world_view_transform() (renderer.py:140-150)."""

    def __init__(self, w, h, fovx, fovy, wv):
        self._width, self._height, self._FoVx, self._FoVy, self._wv = int(w), int(h), float(fovx), float(fovy), wv

    def world_view_transform(self):
        return self._wv


def pose_error(est, true):
    """(rotation angle between the two poses in degrees, distance between the camera centres)."""
    import torch
    Re, Rt = est[:3, :3].double(), true[:3, :3].double()
    cos = ((Re @ Rt.T).trace() - 1.0) / 2.0
    ang = math.degrees(math.acos(float(torch.clamp(cos, -1.0, 1.0))))
    ce, ct = -Re.T @ est[:3, 3].double(), -Rt.T @ true[:3, 3].double()
    return ang, float((ce - ct).norm())


def run(iters: int = 200, n: int = 2000, size: int = 128, lr: float = 2e-3, verbose: bool = True) -> dict:
    import torch
    pkg = _package()
    dev = torch.device("cuda", 0)
    W = H = size
    scene = pkg.synthetic.make_scene(n, W, H, seed=0, sigma_range=(0.05, 0.2))
    model = pkg.synthetic.to_model(scene, pkg.GaussianModel, dev)
    for p in model.parameters():
        p.requires_grad_(False)
    settings = pkg.RenderSettings(image_height=H, image_width=W, bg_color=torch.zeros(3))
    renderer = pkg.GaussianRenderer()

    true = torch.eye(4)
    true[:3, 3] = torch.tensor([0.1, -0.05, 0.3])
    with torch.no_grad():
        target = renderer.render(_Cam(W, H, scene.fovx, scene.fovy, true), model, settings)["image"].clone()
    # the start: 2 degrees and 2 % of the scene's depth (~4) away from the true pose
    axis = torch.tensor([1.0, -1.0, 0.5]) / 1.5
    shift = torch.tensor([-1.0, 0.5, 1.0]) / 1.5
    start = pkg.se3_exp(torch.cat([0.08 * shift, math.radians(2.0) * axis])) @ true
    pose = pkg.CameraPose(_Cam(W, H, scene.fovx, scene.fovy, start))
    opt = torch.optim.Adam(pose.parameters(), lr=lr)

    log = []
    for it in range(iters + 1):
        opt.zero_grad()
        loss = ((renderer.render(pose, model, settings)["image"] - target) ** 2).mean()
        if it % 20 == 0 or it == iters:
            ang, dist = pose_error(pose.world_view_transform().detach(), true)
            log.append((it, loss.item(), ang, dist))
            if verbose:
                print(f"iter {it:4d}  loss {loss.item():.3e}  rotation error {ang:.4f} deg  centre error {dist:.5f}")
        if it < iters:
            loss.backward()
            opt.step()
    return {"log": log, "loss_ratio": log[-1][1] / log[0][1], "angle_ratio": log[-1][2] / log[0][2],
            "centre_ratio": log[-1][3] / log[0][3]}


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--gaussians", type=int, default=2000)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--lr", type=float, default=2e-3)
    a = ap.parse_args()
    r = run(a.iters, a.gaussians, a.size, a.lr)
    print(f"loss x {r['loss_ratio']:.3g}, rotation error x {r['angle_ratio']:.3g}, centre error x {r['centre_ratio']:.3g}")
