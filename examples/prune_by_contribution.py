"""Contribution pruning: train the synthetic stand-in scene briefly, drop every
Gaussian whose largest blend weight over all training views stays below a
threshold (RadSplat's importance score, max_p c_i(p)), and show that the test
PSNR barely moves while the model shrinks.

    stats = gaussians.contribution_stats
    renderer.render(camera, gaussians, settings, contribution_stats=stats)   # per view, no backward
    optimizer.prune_by_contribution(stats, 0.01)                             # Adam moments follow

GaussianTrainer.compact() does the three steps over the training cameras (and
all-reduces the statistics under data parallel); TrainingConfig's
contribution_prune_iterations runs it inside train().  The per-pixel opposite
direction, render(..., dominant=True), gives each pixel's strongest
contributor: written here as <out>/dominant.npy (int32 [H, W], -1 = none) and
<out>/dominant.ppm (one colour per Gaussian).

    python examples/prune_by_contribution.py [--iters 300] [--views 24] [--size 128] [--threshold 0.01]

Needs a HIP device (the renderer has no CPU path).
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run(iters: int = 300, views: int = 24, size: int = 128, threshold: float = 0.01, points: int = 20_000,
        out_dir: str | None = None, verbose: bool = True) -> dict:
    import numpy as np
    import torch
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import __graft_entry__ as ge
    from train_synthetic import build_scene
    pkg = ge.load_package()
    ds = build_scene(pkg, views, size, gt_gaussians=5000)
    out_dir = out_dir or tempfile.mkdtemp()
    cfg = pkg.TrainingConfig(iterations=iters, num_random_points=points, log_interval=max(iters // 5, 1),
                             densify_from_iter=iters + 1, output_path=os.path.join(out_dir, "ckpt"),
                             position_lr_init=1.6e-3, position_lr_final=1.6e-5)
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    tr.train()
    before = tr.validate()
    info = tr.compact(threshold)
    after = tr.validate()
    if verbose:
        print(f"trained {iters} iterations on {len(ds.get_train_cameras())} views of {size}x{size}")
        print(f"before: N = {info['n_before']:6d}  test PSNR {before['psnr']:.2f} dB")
        print(f"after : N = {info['n_after']:6d}  test PSNR {after['psnr']:.2f} dB   (max blend weight > {threshold})")
    # each pixel's strongest contributor in the first training view
    cam = ds.get_train_cameras()[0]
    with torch.no_grad():
        r = tr.renderer.render(cam, tr.gaussians, tr._settings(cam), dominant=True)
    dom = r["dominant_gaussian"].cpu().numpy()
    os.makedirs(out_dir, exist_ok=True)
    np.save(os.path.join(out_dir, "dominant.npy"), dom)
    palette = np.random.default_rng(0).integers(32, 256, (info["n_after"] + 1, 3), dtype=np.uint8)
    palette[-1] = 0  # (id -1: no contributor)
    with open(os.path.join(out_dir, "dominant.ppm"), "wb") as fh:
        fh.write(b"P6 %d %d 255\n" % (dom.shape[1], dom.shape[0]))
        fh.write(palette[dom].tobytes())
    if verbose:
        print(f"dominant-Gaussian map of view 0: {len(np.unique(dom[dom >= 0]))} Gaussians lead a pixel, "
              f"{int((dom < 0).sum())} empty pixels -> {out_dir}/dominant.npy, dominant.ppm")
    return {"n_before": info["n_before"], "n_after": info["n_after"], "psnr_before": before["psnr"],
            "psnr_after": after["psnr"], "out_dir": out_dir}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--views", type=int, default=24)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--threshold", type=float, default=0.01)
    ap.add_argument("--points", type=int, default=20_000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = run(a.iters, a.views, a.size, a.threshold, a.points, a.out)
    assert r["n_after"] < r["n_before"], r


if __name__ == "__main__":
    main()
