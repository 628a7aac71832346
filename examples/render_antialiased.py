"""Anti-aliased rendering: one model drawn at full and at a quarter of the
resolution, with and without the screen-space low-pass filter, and the four
images saved.

RenderSettings(screen_filter=s) adds s (px^2) to every projected covariance,
cov2d + s I, and with filter_compensate=True (the default) scales each opacity
by sqrt(det cov2d / det(cov2d + s I)), so that a splat smaller than a pixel
spreads over the pixel instead of shining on whichever pixel centre it meets:

    settings = RenderSettings(H // 4, W // 4, bg, screen_filter=0.3)
    out = renderer.render(camera_at_quarter_size, model, settings)

    python examples/render_antialiased.py [--gaussians 20000] [--size 512] [--out-dir .]

Writes full.png, full_filtered.png, quarter.png, quarter_filtered.png and
prints each quarter-size image's RMSE against the box-averaged full-size render
(what a camera of that resolution would see).  Needs a HIP device.
"""
from __future__ import annotations

import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


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


def run(n: int = 20000, size: int = 512, variance: float = 0.3, out_dir: str | None = None,
        verbose: bool = True) -> dict:
    import torch
    from simple_scene import _write_png
    pkg = _package()
    dev = torch.device("cuda", 0)
    assert size % 4 == 0
    # splats of about a pixel at full size: a quarter of one at the low resolution
    scene = pkg.synthetic.make_scene(n, size, size, seed=0, sigma_range=(0.002, 0.01))
    model = pkg.synthetic.to_model(scene, pkg.GaussianModel, dev)
    renderer = pkg.GaussianRenderer()
    bg = torch.zeros(3)
    images = {}
    with torch.no_grad():
        for name, edge in (("full", size), ("quarter", size // 4)):
            cam = _Cam(edge, edge, scene.fovx, scene.fovy)  # the same field of view on fewer pixels
            for suffix, s in (("", 0.0), ("_filtered", variance)):
                settings = pkg.RenderSettings(edge, edge, bg, screen_filter=s, filter_compensate=True)
                images[name + suffix] = renderer.render(cam, model, settings)["image"].clamp(0, 1)
    if out_dir is not None:
        os.makedirs(out_dir, exist_ok=True)
        for name, img in images.items():
            _write_png(os.path.join(out_dir, name + ".png"), img.cpu().numpy())
    # what a quarter-resolution camera sees: each of its pixels the mean of the 4x4 full-size ones
    want = torch.nn.functional.avg_pool2d(images["full"][None], 4)[0]
    rmse = {k: float(((images[k] - want) ** 2).mean().sqrt()) for k in ("quarter", "quarter_filtered")}
    if verbose:
        print(f"RMSE against the box-averaged full-size render: unfiltered {rmse['quarter']:.4f}, "
              f"filtered (s = {variance}) {rmse['quarter_filtered']:.4f}")
    return {"rmse_unfiltered": rmse["quarter"], "rmse_filtered": rmse["quarter_filtered"],
            "images": sorted(images)}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--gaussians", type=int, default=20000)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--variance", type=float, default=0.3)
    ap.add_argument("--out-dir", default=".")
    a = ap.parse_args()
    r = run(a.gaussians, a.size, a.variance, a.out_dir)
    assert r["rmse_filtered"] < r["rmse_unfiltered"], r


if __name__ == "__main__":
    main()
