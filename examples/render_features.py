"""Per-Gaussian feature channels: render a one-hot instance palette of the
synthetic scene next to its colour image, then fit a small feature tensor to a
target feature image with a torch optimiser.

render(camera, gaussians, settings, features=F) composites F [N, C] with
exactly the weights the colour pass gave each pixel's contributors
(gs_blend_features_forward) and returns it as out["features"] [C, H, W]; the
backward (gs_blend_features_backward) returns dL/dF and adds the features'
share of the geometry gradient to the colour pass's:

    out = renderer.render(camera, gaussians, settings, features=F)
    loss = ((out["features"] - target) ** 2).mean()
    loss.backward(); opt.step()

    python examples/render_features.py [--iters 60] [--gaussians 2000] [--size 128] [--classes 5]

Prints the feature loss every 10 iterations and how often the rendered arg-max
class matches the target's.  Needs a HIP device (the renderer has no CPU path).
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _package():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    return ge.load_package()


class _Cam:
    """camera._width/_height/_FoVx/_FoVy and world_view_transform() (renderer.py:140-150)."""

    def __init__(self, w, h, fovx, fovy):
        self._width, self._height, self._FoVx, self._FoVy = int(w), int(h), float(fovx), float(fovy)

    def world_view_transform(self):
        import torch
        return torch.eye(4)


def run(iters: int = 60, n: int = 2000, size: int = 128, classes: int = 5, lr: float = 0.1,
        verbose: bool = True) -> dict:
    import torch
    pkg = _package()
    dev = torch.device("cuda", 0)
    W = H = size
    scene = pkg.synthetic.make_scene(n, W, H, seed=0, sigma_range=(0.05, 0.2))
    model = pkg.synthetic.to_model(scene, pkg.GaussianModel, dev)
    cam = _Cam(W, H, scene.fovx, scene.fovy)
    settings = pkg.RenderSettings(H, W, torch.zeros(3))
    renderer = pkg.GaussianRenderer()
    # the target: each Gaussian's instance as a one-hot row, by the octant-like cell of its position
    xyz = model.get_xyz.detach()
    ids = (torch.floor((xyz[:, 0] - xyz[:, 0].min()) / (xyz[:, 0].max() - xyz[:, 0].min() + 1e-6) * classes)
           .long().clamp(0, classes - 1))
    palette = torch.nn.functional.one_hot(ids, classes).float()
    with torch.no_grad():
        ref = renderer.render(cam, model, settings, features=palette)
    target, colour = ref["features"], ref["image"]
    assert target.shape == (classes, H, W) and colour.shape == (3, H, W)
    # what alpha is to the colour image, the channel sum is to a one-hot palette
    assert torch.allclose(target.sum(0), ref["alpha"][0], atol=1e-5)
    # fit: start from zeros, recover the palette from the feature image alone
    F = torch.zeros((n, classes), device=dev, requires_grad=True)
    opt = torch.optim.Adam([F], lr=lr)
    first = last = None
    for it in range(iters):
        opt.zero_grad(set_to_none=True)
        out = renderer.render(cam, model, settings, features=F)  # (the model's .grad fills too; only F is stepped)
        loss = ((out["features"] - target) ** 2).mean()
        loss.backward()
        opt.step()
        last = float(loss)
        first = last if first is None else first
        if verbose and (it % 10 == 0 or it == iters - 1):
            print(f"iter {it:4d}  feature loss {last:.3e}")
    covered = ref["alpha"][0] > 0.5
    agree = float((out["features"].argmax(0) == target.argmax(0))[covered].float().mean()) if covered.any() else 1.0
    if verbose:
        print(f"arg-max class agrees with the target on {100 * agree:.1f} % of the covered pixels")
    return {"first_loss": first, "last_loss": last, "argmax_agreement": agree, "channels": classes}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=60)
    ap.add_argument("--gaussians", type=int, default=2000)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--classes", type=int, default=5)
    a = ap.parse_args()
    r = run(a.iters, a.gaussians, a.size, a.classes)
    assert r["last_loss"] < 0.2 * r["first_loss"], r


if __name__ == "__main__":
    main()
