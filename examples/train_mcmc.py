"""3DGS-MCMC density control (densify_criterion = "mcmc") on the synthetic scene
of examples/simple_scene.py: the 5k random Gaussians of config C1 are the
ground truth, seen from a ring of cameras, and a model of `--points` random
Gaussians is trained towards them.

    cfg = TrainingConfig(densify_criterion="mcmc", mcmc_cap_max=6000, ...)
    GaussianTrainer(cfg, dataset).train()

Nothing is split, cloned or pruned.  Every densify_interval iterations the
Gaussians whose opacity fell to mcmc_min_opacity are relocated onto live ones
(drawn in proportion to their opacity, the copies sharing the source's opacity
and scale so that the render is preserved) and N grows by 5 % up to
mcmc_cap_max; from then on no parameter or Adam moment is reallocated.  Every
iteration adds opacity-gated noise to the positions and the opacity / scale
regularisers to the gradients.

    python examples/train_mcmc.py [--iters 600] [--views 16] [--size 128] [--points 4000] [--cap 6000]

Needs a HIP device (the renderer has no CPU path).
"""
from __future__ import annotations

import argparse
import math
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_dataset(pkg, views: int, size: int, device):
    """simple_scene.py's model rendered from `views` cameras on a ring of radius 3 around it."""
    import numpy as np
    import torch
    gt = pkg.GaussianModel(pkg.TrainingConfig())
    gt.create_from_random(5000, scene_extent=1.0, device=device, generator=torch.Generator().manual_seed(0))
    with torch.no_grad():
        gen = torch.Generator().manual_seed(1)
        gt._scaling.add_((torch.rand(gt._scaling.shape, generator=gen) - 0.5).to(device))
        gt._opacity.copy_(torch.randn(gt._opacity.shape, generator=gen).to(device))
    ds = pkg.CameraDataset("", device=device)
    renderer = pkg.GaussianRenderer()
    settings = pkg.RenderSettings(image_height=size, image_width=size, bg_color=torch.zeros(3))
    for i in range(views):
        th = 2.0 * math.pi * i / views
        c, s = math.cos(th), math.sin(th)
        R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], np.float32)  # camera-to-world; +z looks at the origin
        cam = pkg.Camera(uid=i, R=R, T=-3.0 * R[:, 2], FoVx=math.radians(60), FoVy=math.radians(60), image=None,
                         image_name=f"ring_{i}", width=size, height=size)
        with torch.no_grad():
            cam._image = renderer.render(cam, gt, settings)["image"].clone()
        ds.cameras.append(cam)
    ds.split_train_test(0.25)
    return ds


def run(iters: int = 600, views: int = 16, size: int = 128, points: int = 4000, cap: int = 6000,
        out_dir: str | None = None, verbose: bool = True) -> dict:
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    ds = build_dataset(pkg, views, size, dev)
    out_dir = out_dir or tempfile.mkdtemp()
    interval = max(iters // 12, 1)
    cfg = pkg.TrainingConfig(iterations=iters, num_random_points=points, log_interval=max(iters // 6, 1),
                             densify_criterion="mcmc", densify_from_iter=interval, densify_until_iter=iters + interval,
                             densify_interval=interval, mcmc_cap_max=cap, mcmc_noise_lr=5e4,
                             output_path=os.path.join(out_dir, "ckpt"), position_lr_init=1.6e-3,
                             position_lr_final=1.6e-5)
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    before = tr.validate()
    history = []
    for _ in range(iters):
        tr.train(1)
        if tr.iteration % interval == 0:
            history.append(dict(tr.last_densify, iteration=tr.iteration))
    after = tr.validate()
    ptrs = [p.data_ptr() for p in tr.gaussians.parameter_list()]
    tr.train(interval)  # one more refinement at the cap: in place
    in_place = ptrs == [p.data_ptr() for p in tr.gaussians.parameter_list()]
    if verbose:
        print(f"{len(ds.get_train_cameras())} training views of {size}x{size}, {iters} iterations, cap {cap}")
        for h in history:
            print(f"  iteration {h['iteration']:5d}: relocated {h['relocated']:5d}, added {h['added']:4d}, N = {h['n']}")
        print(f"test PSNR {before['psnr']:.2f} -> {after['psnr']:.2f} dB, N = {points} -> {after['num_gaussians']}; "
              f"parameters stay in place at the cap: {in_place}")
    return {"psnr_before": before["psnr"], "psnr_after": after["psnr"], "n": after["num_gaussians"],
            "history": history, "in_place_at_cap": in_place}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=600)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--cap", type=int, default=6000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = run(a.iters, a.views, a.size, a.points, a.cap, a.out)
    assert r["n"] <= a.cap and r["psnr_after"] > r["psnr_before"], r


if __name__ == "__main__":
    main()
