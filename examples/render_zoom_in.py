"""Zoom-in with Mip-Splatting's 3D smoothing filter: the synthetic scene of
examples/train_mcmc.py is trained at a quarter of the resolution, once without
and once with TrainingConfig(filter_3d=True), and both models are then rendered
at the full resolution -- four times the focal length of any training view.

    cfg = TrainingConfig(filter_3d=True, filter_3d_variance=0.2, ...)
    trainer = GaussianTrainer(cfg, dataset); trainer.train()
    renderer.render(camera, trainer.gaussians, settings, filter_3d=trainer.filter_3d)

The filter bounds every Gaussian's size from below by the highest sampling rate
a training camera saw it at, so a model fitted to coarse images cannot hide
needle-thin splats that only a closer look reveals.  To bake it into a model
for export: scaling', opacity' = apply_filter_3d(model._scaling,
model._opacity, trainer.filter_3d.values).

    python examples/render_zoom_in.py [--iters 600] [--views 16] [--size 256] [--points 4000]

Prints both models' RMSE against the full-resolution ground truth (a report:
on a haze of random Gaussians the outcome is not known in advance).  Needs a
HIP device.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def run(iters: int = 600, views: int = 16, size: int = 256, points: int = 4000, variance: float = 0.2,
        out_dir: str | None = None, verbose: bool = True) -> dict:
    import torch
    from train_mcmc import build_dataset
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    assert size % 4 == 0
    low = build_dataset(pkg, views, size // 4, dev)   # the training views
    full = build_dataset(pkg, views, size, dev)       # the same cameras on four times the pixels
    out_dir = out_dir or tempfile.mkdtemp()
    interval = max(iters // 6, 1)
    renderer = pkg.GaussianRenderer()
    res = {}
    for name, on in (("plain", False), ("filter_3d", True)):
        cfg = pkg.TrainingConfig(iterations=iters, num_random_points=points, log_interval=max(iters // 6, 1),
                                 densify_from_iter=interval, densify_until_iter=iters // 2, densify_interval=interval,
                                 output_path=os.path.join(out_dir, name), position_lr_init=1.6e-3,
                                 position_lr_final=1.6e-5, filter_3d=on, filter_3d_variance=variance)
        tr = pkg.GaussianTrainer(cfg, low)
        tr.train()
        kw = {"filter_3d": tr.filter_3d} if on else {}
        err = {}
        with torch.no_grad():
            for key, ds in (("train_resolution", low), ("zoom_in", full)):
                mse = [((renderer.render(c, tr.gaussians, tr._settings(c), **kw)["image"] - c._image) ** 2).mean()
                       for c in ds.cameras]
                err[key] = float(torch.stack(mse).mean().sqrt())
        res[name] = dict(err, n=tr.gaussians.get_num_points())
        if verbose:
            print(f"{name:10s}: N = {res[name]['n']}, RMSE at the training resolution {err['train_resolution']:.4f}, "
                  f"at four times the focal length {err['zoom_in']:.4f}")
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--iters", type=int, default=600)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--variance", type=float, default=0.2)
    a = ap.parse_args()
    run(a.iters, a.views, a.size, a.points, a.variance)


if __name__ == "__main__":
    main()
