"""The depth distortion loss (TrainingConfig.lambda_distortion) on the synthetic
scene of examples/train_mcmc.py: the 5k random Gaussians of config C1 are the
ground truth, seen from a ring of cameras, and a model of `--points` random
Gaussians is trained towards them twice, without and with the term.

    cfg = TrainingConfig(lambda_distortion=1.0, distortion_from_iter=100, ...)
    GaussianTrainer(cfg, dataset).train()

From distortion_from_iter on the loss is photometric + lambda_distortion *
out["distortion"].mean(), where out["distortion"][p] = sum_ij c_i c_j |z_i - z_j|
over pixel p's contributors (render(..., depth_distortion=True)): it pulls
each ray's weights into one thin shell.  Both runs print the mean distortion
over the test views and the test PSNR; the median-depth image of the first
test view of the second run is written as a PGM file.

    python examples/train_distortion.py [--iters 600] [--views 16] [--size 128] [--points 4000] [--lam 1]

Needs a HIP device (the renderer has no CPU path).
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))


def mean_distortion(tr, cams) -> float:
    import torch
    with torch.no_grad():
        d = [tr.renderer.render(c, tr.gaussians, tr._settings(c), depth_distortion=True)["distortion"].mean()
             for c in cams]
    return float(torch.stack(d).mean())


def write_pgm(path: str, depth) -> None:
    """An 8-bit PGM of a depth map: nearest = white, farthest = dark, no contributor = black."""
    import numpy as np
    z = depth.cpu().numpy()
    hit = z > 0
    img = np.zeros(z.shape, np.uint8)
    if hit.any():
        lo, hi = float(z[hit].min()), float(z[hit].max())
        img[hit] = (255.0 - 200.0 * (z[hit] - lo) / max(hi - lo, 1e-12)).astype(np.uint8)
    with open(path, "wb") as f:
        f.write(b"P5 %d %d 255\n" % (z.shape[1], z.shape[0]))
        f.write(img.tobytes())


def run(iters: int = 600, views: int = 16, size: int = 128, points: int = 4000, lam: float = 1.0,
        out_dir: str | None = None, verbose: bool = True) -> dict:
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    from train_mcmc import build_dataset
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    ds = build_dataset(pkg, views, size, dev)
    out_dir = out_dir or tempfile.mkdtemp()
    os.makedirs(out_dir, exist_ok=True)
    tests = ds.get_test_cameras() or ds.get_train_cameras()
    res = {}
    for name, weight in (("plain", 0.0), ("distortion", lam)):
        cfg = pkg.TrainingConfig(iterations=iters, num_random_points=points, log_interval=max(iters // 6, 1),
                                 densify_from_iter=10 ** 9, densify_until_iter=10 ** 9,
                                 lambda_distortion=weight, distortion_from_iter=iters // 6,
                                 output_path=os.path.join(out_dir, "ckpt_" + name), position_lr_init=1.6e-3,
                                 position_lr_final=1.6e-5)
        tr = pkg.GaussianTrainer(cfg, ds)
        tr.setup()
        tr.train(iters)
        res[name] = {"psnr": tr.validate()["psnr"], "mean_distortion": mean_distortion(tr, tests)}
    with torch.no_grad():
        out = tr.renderer.render(tests[0], tr.gaussians, tr._settings(tests[0]), depth_distortion=True)
    path = os.path.join(out_dir, "median_depth.pgm")
    write_pgm(path, out["median_depth"])
    res["median_depth_image"] = path
    if verbose:
        print(f"{len(ds.get_train_cameras())} training views of {size}x{size}, {iters} iterations, {points} Gaussians")
        for name in ("plain", "distortion"):
            print(f"  {name:10s}: mean distortion {res[name]['mean_distortion']:.4g}, test PSNR {res[name]['psnr']:.2f} dB")
        print(f"median depth of the first test view: {path}")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=600)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--points", type=int, default=4000)
    ap.add_argument("--lam", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = run(a.iters, a.views, a.size, a.points, a.lam, a.out)
    assert r["distortion"]["mean_distortion"] < r["plain"]["mean_distortion"], r


if __name__ == "__main__":
    main()
