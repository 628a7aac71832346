"""Bilateral-grid appearance compensation (TrainingConfig.bilateral_grid) on a
synthetic capture with changing exposure and white balance: a ball of
Gaussians is the ground truth, seen from a ring of cameras, and every training
image is multiplied by its own gain and white balance (per-channel factors
from [1 - spread, 1 + spread]) -- what auto-exposure does to a real capture.
A model of `--points` random Gaussians is trained towards it twice, without
and with the option.

    cfg = TrainingConfig(bilateral_grid=True, ...)
    GaussianTrainer(cfg, dataset).train()

With the option every training camera owns a 16 x 16 x 8 grid of affine colour
transforms; the step's render is sliced through its camera's grid
(slice_bilateral_grid) before the photometric loss, which also gains lambda_tv
* bilateral_grid_tv(grid).  Both runs print the mean photometric loss over the
training views, each view through its own pipeline (the run with the grids
corrects its render with the view's grid, as its training step does), and the
PSNR of the uncorrected renders against the clean images of the held-out views.
The grids are free up to one common colour transform, so the second number
may move either way; the first is what the option is for.

    python examples/train_bilateral_grid.py [--iters 600] [--views 16] [--size 96] [--points 3000] [--spread 0.4]

Needs a HIP device (the renderer has no CPU path).
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_dataset(pkg, views: int, size: int, spread: float, device):
    """1500 Gaussians in a ball of radius 0.7, rendered from `views` cameras on
    a ring of radius 4; every fourth view is held out with its clean image, the
    others are multiplied by their own per-channel gain."""
    import numpy as np
    import torch
    g = torch.Generator().manual_seed(3)
    n = 1500
    d = torch.randn(n, 3, generator=g)
    xyz = d / d.norm(dim=1, keepdim=True) * 0.7 * torch.rand(n, 1, generator=g) ** (1 / 3)
    gt = pkg.GaussianModel(pkg.TrainingConfig())
    gt._set(xyz.to(device), (torch.rand(n, 1, 3, generator=g) * 4 - 2).to(device), torch.zeros(n, 15, 3, device=device),
            torch.log(0.03 + 0.05 * torch.rand(n, 3, generator=g)).to(device),
            torch.nn.functional.normalize(torch.randn(n, 4, generator=g), dim=-1).to(device),
            torch.full((n, 1), 1.5, device=device))
    ds = pkg.CameraDataset("", device=device)
    renderer = pkg.GaussianRenderer()
    settings = pkg.RenderSettings(image_height=size, image_width=size, bg_color=torch.zeros(3))
    for i in range(views):
        th = 2 * math.pi * i / views
        c, s = math.cos(th), math.sin(th)
        R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], np.float32)  # camera-to-world; +z looks at the origin
        cam = pkg.Camera(uid=i, R=R, T=-4.0 * R[:, 2], FoVx=math.radians(40), FoVy=math.radians(40), image=None,
                         image_name=f"ring_{i}", width=size, height=size)
        with torch.no_grad():
            cam._image = renderer.render(cam, gt, settings)["image"].clone()
        ds.cameras.append(cam)
    ds.split_train_test(0.25)
    gains = 1 + spread * (2 * torch.rand(len(ds.get_train_cameras()), 3, generator=g) - 1)
    for cam, gain in zip(ds.get_train_cameras(), gains):
        cam._image = cam._image * gain.to(device)[:, None, None]
    return ds


def mean_train_loss(pkg, tr) -> float:
    import torch
    losses = []
    with torch.no_grad():
        for i, cam in enumerate(tr.dataset.get_train_cameras()):
            img = tr.renderer.render(cam, tr.gaussians, tr._settings(cam))["image"]
            if tr.bilagrid is not None:
                img = tr.bilagrid.slice(i, img)
            losses.append(pkg.photometric_loss(img, cam._image, tr.config.lambda_dssim)[0])
    return float(torch.stack(losses).mean())


def run(iters: int = 600, views: int = 16, size: int = 96, points: int = 3000, spread: float = 0.4,
        out_dir: str | None = None, verbose: bool = True) -> dict:
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    ds = build_dataset(pkg, views, size, spread, dev)
    out_dir = out_dir or tempfile.mkdtemp()
    res = {}
    for name, on in (("plain", False), ("grids", True)):
        cfg = pkg.TrainingConfig(iterations=iters, num_random_points=points, log_interval=max(iters // 6, 1),
                                 densify_from_iter=10 ** 9, densify_until_iter=10 ** 9, bilateral_grid=on,
                                 bilateral_grid_lr=1e-2, bilateral_grid_warmup=max(iters // 20, 1),
                                 output_path=os.path.join(out_dir, "ckpt_" + name), position_lr_init=1.6e-3,
                                 position_lr_final=1.6e-5)
        tr = pkg.GaussianTrainer(cfg, ds)
        tr.setup()
        tr.train(iters)
        res[name] = {"train_loss": mean_train_loss(pkg, tr), "test_psnr": tr.validate()["psnr"]}
    if verbose:
        print(f"{len(ds.get_train_cameras())} training views of {size}x{size} with gains in [{1 - spread:.2f}, "
              f"{1 + spread:.2f}], {iters} iterations, {points} Gaussians")
        for name in ("plain", "grids"):
            r = res[name]
            print(f"  {name:5s}: mean training loss {r['train_loss']:.5f}, test PSNR (uncorrected render, clean "
                  f"image) {r['test_psnr']:.2f} dB")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=600)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--spread", type=float, default=0.4)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = run(a.iters, a.views, a.size, a.points, a.spread, a.out)
    assert r["grids"]["train_loss"] < r["plain"]["train_loss"], r
    assert all(math.isfinite(v) for run_ in r.values() for v in run_.values()), r


if __name__ == "__main__":
    main()
