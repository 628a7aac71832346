"""Density control on absolute screen-space gradients (AbsGS; gsplat's absgrad)
on the synthetic scene of examples/simple_scene.py: the 5k random Gaussians of
config C1 are the ground truth, seen from a ring of cameras, and a model of
`--points` random Gaussians is trained towards them.

    cfg = TrainingConfig(densify_criterion="screen", densify_absgrad=True,
                         densify_abs_grad_threshold=0.0008, ...)
    GaussianTrainer(cfg, dataset).train()

Every render's backward adds the view to gaussians.density_stats: the signed
statistic (the norm of dL/d(projected centre), whose per-pixel terms can cancel
over a large Gaussian) and the absolute one (the same norm of the per-pixel
absolute gradients, which cannot).  At a densification large Gaussians split
where the mean absolute gradient exceeds densify_abs_grad_threshold, small ones
clone where the signed mean exceeds densify_grad_threshold.  `--no-absgrad`
trains the plain "screen" criterion on the same scene for comparison.

    python examples/train_absgrad.py [--iters 600] [--views 16] [--size 128] [--points 2000] [--no-absgrad]

Needs a HIP device (the renderer has no CPU path).
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from train_mcmc import build_dataset  # noqa: E402  (the same scene and cameras)


def run(iters: int = 600, views: int = 16, size: int = 128, points: int = 2000, absgrad: bool = True,
        abs_threshold: float = 0.0008, out_dir: str | None = None, verbose: bool = True) -> dict:
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    ds = build_dataset(pkg, views, size, dev)
    out_dir = out_dir or tempfile.mkdtemp()
    interval = max(iters // 6, 1)
    cfg = pkg.TrainingConfig(iterations=iters, num_random_points=points, log_interval=max(iters // 6, 1),
                             densify_criterion="screen", densify_absgrad=absgrad,
                             densify_abs_grad_threshold=abs_threshold, densify_from_iter=interval,
                             densify_until_iter=iters - interval, densify_interval=interval,
                             output_path=os.path.join(out_dir, "ckpt"), position_lr_init=1.6e-3,
                             position_lr_final=1.6e-5)
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    before = tr.validate()
    history = []
    for _ in range(iters):
        if tr.optimizer.density_controller.should_densify(tr.iteration + 1):
            # (the statistics the coming densification reads: they restart as zeros after it)
            st = tr.gaussians.density_stats
            seen = st.denom > 0
            means = {"signed": float(st.mean_grad()[seen].mean())}
            if absgrad:
                means["abs"] = float(st.mean_abs_grad()[seen].mean())
        tr.train(1)
        if tr.optimizer.density_controller.should_densify(tr.iteration):
            history.append(dict(tr.last_densify, iteration=tr.iteration, **means))
    after = tr.validate()
    if verbose:
        rule = "screen + absgrad" if absgrad else "screen"
        print(f"{len(ds.get_train_cameras())} training views of {size}x{size}, {iters} iterations, criterion {rule}")
        for h in history:
            stat = f"mean signed {h['signed']:.3g}" + (f", abs {h['abs']:.3g}" if absgrad else "")
            print(f"  iteration {h['iteration']:5d}: {stat}; split {h['split']:5d}, cloned {h['cloned']:5d}, N = {h['n']}")
        print(f"test PSNR {before['psnr']:.2f} -> {after['psnr']:.2f} dB, N = {points} -> {after['num_gaussians']}")
    return {"psnr_before": before["psnr"], "psnr_after": after["psnr"], "n": after["num_gaussians"], "history": history}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=600)
    ap.add_argument("--views", type=int, default=16)
    ap.add_argument("--size", type=int, default=128)
    ap.add_argument("--points", type=int, default=2000)
    ap.add_argument("--abs-threshold", type=float, default=0.0008)
    ap.add_argument("--no-absgrad", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = run(a.iters, a.views, a.size, a.points, not a.no_absgrad, a.abs_threshold, a.out)
    assert r["psnr_after"] > r["psnr_before"], r
    assert a.no_absgrad or all("abs" in h for h in r["history"])


if __name__ == "__main__":
    main()
