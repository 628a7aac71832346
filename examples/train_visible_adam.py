"""Visibility-gated Adam (gsplat's visible_adam, the sparse Adam of Taming 3DGS)
on a scene several times wider than one view: a slab of random Gaussians,
`--width` units long and 2 x 2 across, seen by a row of cameras that look at it
side on from 4 units off its axis, each covering about 4.6 units of its length.

    cfg = TrainingConfig(visible_adam=True, ...)
    GaussianTrainer(cfg, dataset).train()

A step's view sees a fraction of the model.  The dense Adam step still updates
every Gaussian: one outside the view has a zero gradient, but its moments decay
and its parameters keep moving along the stale first moment.  With
visible_adam the step updates the rows of the render's visibility_filter only
and leaves every other row's parameters and moments bit for bit (and their
memory untouched).  The same scene is trained from the same initial points
with the option off and on; the script prints the held-out PSNR of both and the
mean fraction of the model a step saw.

    python examples/train_visible_adam.py [--iters 600] [--views 24] [--size 96] [--points 6000] [--width 16]

Needs a HIP device (the renderer has no CPU path).
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_dataset(pkg, views: int, size: int, width: float, points: int, device):
    """The slab's ground truth rendered from `views` cameras in a row 4 off
    its axis; every fourth camera is held out.  The initial points are the
    ground-truth centres, jittered."""
    import numpy as np
    import torch
    gen = torch.Generator().manual_seed(0)
    n = 1500 * max(int(width) // 4, 1)
    box = torch.tensor([width, 2.0, 2.0])
    xyz = (torch.rand(n, 3, generator=gen) - 0.5) * box
    gt = pkg.GaussianModel(pkg.TrainingConfig())
    gt._set(xyz.to(device), (torch.rand(n, 1, 3, generator=gen) * 4 - 2).to(device), torch.zeros(n, 15, 3, device=device),
            torch.log(0.03 + 0.05 * torch.rand(n, 3, generator=gen)).to(device),
            torch.nn.functional.normalize(torch.randn(n, 4, generator=gen), dim=-1).to(device),
            torch.full((n, 1), 1.5).to(device))
    ds = pkg.CameraDataset("", device=device)
    renderer = pkg.GaussianRenderer()
    settings = pkg.RenderSettings(image_height=size, image_width=size, bg_color=torch.zeros(3))
    for i in range(views):
        x = (i / (views - 1) - 0.5) * (width - 2.0)
        cam = pkg.Camera(uid=i, R=np.eye(3, dtype=np.float32), T=np.array([x, 0.0, -4.0], np.float32),
                         FoVx=math.radians(60), FoVy=math.radians(60), image=None, image_name=f"row_{i}",
                         width=size, height=size)  # (camera-to-world; +z looks at the slab)
        with torch.no_grad():
            cam._image = renderer.render(cam, gt, settings)["image"].clone()
        ds.cameras.append(cam)
    ds.split_train_test(0.25)
    pick = torch.randint(n, (points,), generator=gen)
    ds.points = (xyz[pick] + 0.05 * torch.randn(points, 3, generator=gen)).numpy()
    ds.colors = torch.rand(points, 3, generator=gen).numpy()
    return ds


def train(pkg, ds, iters: int, visible_adam: bool, out_dir: str) -> dict:
    import torch
    cfg = pkg.TrainingConfig(iterations=iters, log_interval=max(iters // 6, 1), densify_from_iter=iters + 1,
                             densify_until_iter=iters + 1, visible_adam=visible_adam,
                             output_path=os.path.join(out_dir, f"ckpt{int(visible_adam)}"), position_lr_init=1.6e-3,
                             position_lr_final=1.6e-5)
    torch.manual_seed(0)  # (the initial rotations are drawn on the device)
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    before = tr.validate()
    seen = torch.zeros((), device=tr.gaussians._xyz.device)
    for _ in range(iters):
        tr.iteration += 1
        cam = tr._camera_for(tr.iteration)
        with torch.no_grad():  # (the fraction the step is about to see; the trainer takes the mask from its own render)
            seen += tr.renderer.render(cam, tr.gaussians, tr._settings(cam))["visibility_filter"].float().mean()
        tr.train_step(cam)
    after = tr.validate()
    return {"psnr_before": before["psnr"], "psnr_after": after["psnr"], "visible_fraction": float(seen) / iters}


def run(iters: int = 600, views: int = 24, size: int = 96, points: int = 6000, width: float = 16.0,
        out_dir: str | None = None, verbose: bool = True) -> dict:
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    ds = build_dataset(pkg, views, size, width, points, dev)
    out_dir = out_dir or tempfile.mkdtemp()
    dense = train(pkg, ds, iters, False, out_dir)
    gated = train(pkg, ds, iters, True, out_dir)
    if verbose:
        print(f"{len(ds.get_train_cameras())} training and {len(ds.get_test_cameras())} held-out views of {size}x{size}, "
              f"a slab {width:g} long, {points} Gaussians, {iters} iterations")
        print(f"  a step's view saw {100 * gated['visible_fraction']:.1f} % of the model on average")
        print(f"  dense Adam:   held-out PSNR {dense['psnr_before']:.2f} -> {dense['psnr_after']:.2f} dB")
        print(f"  visible_adam: held-out PSNR {gated['psnr_before']:.2f} -> {gated['psnr_after']:.2f} dB")
    return {"dense": dense, "visible_adam": gated}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=600)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--points", type=int, default=6000)
    ap.add_argument("--width", type=float, default=16.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = run(a.iters, a.views, a.size, a.points, a.width, a.out)
    for k in ("dense", "visible_adam"):
        assert r[k]["psnr_after"] > r[k]["psnr_before"], r
    assert r["visible_adam"]["visible_fraction"] < 0.5, r


if __name__ == "__main__":
    main()
