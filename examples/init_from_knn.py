"""Start-up scales from the neighbourhood of every point (scale_init = "knn").

    d2 = mean_knn_dist2(points, 3)            # simple_knn's distCUDA2
    model.create_from_points(points, colors, scale_init="knn")
    TrainingConfig(scale_init="knn")

Two things are shown.

1. The search itself, timed with HIP events after a warm-up: `mean_knn_dist2`
   at 100 k and 1 M points, uniform in a cube and clustered -- the clustered
   cloud is a mixture made here, not synthetic.py's scene: 90 % of the points
   in 64 tight clusters (sigma 0.002 in a unit cube), 10 % spread over a box a
   hundred times as wide, the density contrast of an SfM cloud.  Next to it the
   only thing torch offers, chunked `cdist` + `topk` at 100 k (4 TB of
   distances at 1 M).

2. A short training run of the synthetic scene of examples/train_mcmc.py from
   a point cloud -- the ground truth's centres, thinned and jittered, as an SfM
   cloud would give them -- with each scale_init, printing test PSNR and the
   number of Gaussians.

    python examples/init_from_knn.py [--iters 400] [--views 16] [--size 128] [--points 3000] [--no-timing]

Needs a HIP device.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def uniform_cloud(n: int, device, seed: int = 0):
    import torch
    return torch.rand(n, 3, generator=torch.Generator().manual_seed(seed)).to(device)


def clustered_cloud(n: int, device, seed: int = 0):
    """90 % in 64 clusters of sigma 0.002 inside the unit cube, 10 % uniform in [-50, 50]^3."""
    import torch
    g = torch.Generator().manual_seed(seed)
    near = n - n // 10
    centres = torch.rand(64, 3, generator=g)
    pts = centres[torch.randint(0, 64, (near,), generator=g)] + 0.002 * torch.randn(near, 3, generator=g)
    far = (torch.rand(n - near, 3, generator=g) - 0.5) * 100.0
    return torch.cat([pts, far])[torch.randperm(n, generator=g)].to(device)


def time_ms(fn, repeats: int = 5) -> float:
    """Median over `repeats` of one call's HIP-event interval, after a warm-up call."""
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return sorted(times)[len(times) // 2]


def cdist_topk(points, k: int = 3, chunk: int = 4096):
    """What torch offers: O(N^2) distances, a chunk of rows at a time."""
    import torch
    out = torch.empty(points.shape[0], device=points.device)
    for r0 in range(0, points.shape[0], chunk):
        d = torch.cdist(points[r0:r0 + chunk], points)
        out[r0:r0 + chunk] = d.topk(k + 1, dim=1, largest=False).values[:, 1:].square().mean(1)
    return out


def timings(pkg, device, sizes=(100_000, 1_000_000), verbose: bool = True) -> dict:
    out = {}
    for name, make in (("uniform", uniform_cloud), ("clustered", clustered_cloud)):
        for n in sizes:
            pts = make(n, device)
            out[f"{name}_{n}"] = ms = time_ms(lambda: pkg.mean_knn_dist2(pts, 3))
            if verbose:
                print(f"mean_knn_dist2, {name:9s} {n:8d} points: {ms:9.3f} ms")
    pts = uniform_cloud(100_000, device)
    out["cdist_topk_100000"] = ms = time_ms(lambda: cdist_topk(pts), repeats=3)
    if verbose:
        print(f"chunked cdist + topk, uniform {100_000:8d} points: {ms:9.3f} ms")
    return out


def train_both(pkg, device, iters: int, views: int, size: int, points: int, out_dir: str, verbose: bool = True) -> dict:
    import torch
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from train_mcmc import build_dataset
    ds = build_dataset(pkg, views, size, device)
    # the "SfM cloud": centres of the ground truth (simple_scene.py's 5000 Gaussians), thinned and jittered
    gt = pkg.GaussianModel(pkg.TrainingConfig())
    gt.create_from_random(5000, scene_extent=1.0, device="cpu", generator=torch.Generator().manual_seed(0))
    g = torch.Generator().manual_seed(2)
    keep = torch.randperm(5000, generator=g)[:points]
    ds.points = (gt._xyz.detach()[keep] + 0.01 * torch.randn(len(keep), 3, generator=g)).numpy()
    ds.colors = torch.full((len(keep), 3), 0.5).numpy()
    res = {}
    for scale_init in ("extent", "knn"):
        cfg = pkg.TrainingConfig(iterations=iters, log_interval=max(iters // 4, 1), scale_init=scale_init,
                                 densify_criterion="screen", densify_from_iter=iters // 4,
                                 densify_until_iter=iters, densify_interval=max(iters // 8, 1),
                                 output_path=os.path.join(out_dir, scale_init), position_lr_init=1.6e-3,
                                 position_lr_final=1.6e-5)
        tr = pkg.GaussianTrainer(cfg, ds)
        tr.setup()
        before = tr.validate()
        tr.train(iters)
        after = tr.validate()
        res[scale_init] = {"psnr_start": before["psnr"], "psnr": after["psnr"], "n": after["num_gaussians"]}
        if verbose:
            print(f"scale_init={scale_init!r:9s}: test PSNR {before['psnr']:.2f} -> {after['psnr']:.2f} dB after {iters} "
                  f"iterations, N = {len(keep)} -> {after['num_gaussians']}")
    return res


def run(iters: int = 400, views: int = 16, size: int = 128, points: int = 3000, timing: bool = True,
        out_dir: str | None = None, verbose: bool = True) -> dict:
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    res = {"timings_ms": timings(pkg, dev, verbose=verbose) if timing else {}}
    res["training"] = train_both(pkg, dev, iters, views, size, points, out_dir or tempfile.mkdtemp(), verbose)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=400)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--no-timing", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    run(a.iters, a.views, a.size, a.points, not a.no_timing, a.out)


if __name__ == "__main__":
    main()
