"""The normal consistency loss (TrainingConfig.lambda_normal) on a small planar
scene: a textured plane of flat Gaussians is the ground truth, seen from an arc
of cameras in front of it, and a model of `--points` random Gaussians is trained
towards it twice, without and with the term.

    cfg = TrainingConfig(lambda_normal=0.05, normal_from_iter=100, ...)
    GaussianTrainer(cfg, dataset).train()

After normal_from_iter iterations the loss is photometric + lambda_normal *
normal_consistency(out["normals"], out["depth"], out["alpha"], camera).mean(),
where out["normals"] = sum_i c_i n_i (render(..., normals=True)) are the
rendered normals and the error is 1 - alpha (N_r . n_d) against the normal n_d
of the depth map: it turns each splat's flat axis towards the surface the
depth map shows.  Both runs print the mean normal error over the test views
before and after the training, and the test PSNR.

    python examples/train_normal_consistency.py [--iters 600] [--views 12] [--size 96] [--points 3000] [--lam 0.05]

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
    """A 2 x 2 plane through the origin (normal +z) of 40 x 40 flat Gaussians with
    a smooth colour pattern, rendered from `views` cameras on a 100 degree arc
    of radius 3 on its -z side."""
    import numpy as np
    import torch
    k = 40
    u, v = torch.meshgrid(torch.linspace(-1, 1, k), torch.linspace(-1, 1, k), indexing="ij")
    n = k * k
    xyz = torch.stack([u.reshape(-1), v.reshape(-1), torch.zeros(n)], 1)
    colour = torch.stack([torch.sin(3 * u), torch.cos(4 * v), torch.sin(2 * (u + v))], -1).reshape(n, 1, 3) * 2
    gt = pkg.GaussianModel(pkg.TrainingConfig())
    gt._set(xyz.to(device), colour.to(device), torch.zeros(n, 15, 3, device=device),
            torch.log(torch.tensor([0.04, 0.04, 0.0004])).repeat(n, 1).to(device),
            torch.tensor([1.0, 0, 0, 0]).repeat(n, 1).to(device), torch.full((n, 1), 3.0, device=device))
    ds = pkg.CameraDataset("", device=device)
    renderer = pkg.GaussianRenderer()
    settings = pkg.RenderSettings(image_height=size, image_width=size, bg_color=torch.zeros(3))
    for i in range(views):
        th = math.radians(-50 + 100 * i / max(views - 1, 1))
        c, s = math.cos(th), math.sin(th)
        R = np.array([[c, 0.0, s], [0.0, 1.0, 0.0], [-s, 0.0, c]], np.float32)  # camera-to-world; +z looks at the origin
        cam = pkg.Camera(uid=i, R=R, T=-3.0 * R[:, 2], FoVx=math.radians(50), FoVy=math.radians(50), image=None,
                         image_name=f"arc_{i}", width=size, height=size)
        with torch.no_grad():
            cam._image = renderer.render(cam, gt, settings)["image"].clone()
        ds.cameras.append(cam)
    ds.split_train_test(0.25)
    return ds


def mean_normal_error(pkg, tr, cams) -> float:
    import torch
    with torch.no_grad():
        e = []
        for c in cams:
            out = tr.renderer.render(c, tr.gaussians, tr._settings(c), normals=True)
            e.append(pkg.normal_consistency(out["normals"], out["depth"], out["alpha"], c).mean())
    return float(torch.stack(e).mean())


def run(iters: int = 600, views: int = 12, size: int = 96, points: int = 3000, lam: float = 0.05,
        out_dir: str | None = None, verbose: bool = True) -> dict:
    import torch
    sys.path.insert(0, ROOT)
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda", 0)
    ds = build_dataset(pkg, views, size, dev)
    out_dir = out_dir or tempfile.mkdtemp()
    tests = ds.get_test_cameras() or ds.get_train_cameras()
    res = {}
    for name, weight in (("plain", 0.0), ("normal", lam)):
        cfg = pkg.TrainingConfig(iterations=iters, num_random_points=points, log_interval=max(iters // 6, 1),
                                 densify_from_iter=10 ** 9, densify_until_iter=10 ** 9,
                                 lambda_normal=weight, normal_from_iter=iters // 6,
                                 output_path=os.path.join(out_dir, "ckpt_" + name), position_lr_init=1.6e-3,
                                 position_lr_final=1.6e-5)
        tr = pkg.GaussianTrainer(cfg, ds)
        tr.setup()
        before = mean_normal_error(pkg, tr, tests)
        tr.train(iters)
        res[name] = {"before": before, "after": mean_normal_error(pkg, tr, tests), "psnr": tr.validate()["psnr"]}
    if verbose:
        print(f"{len(ds.get_train_cameras())} training views of {size}x{size}, {iters} iterations, {points} Gaussians")
        for name in ("plain", "normal"):
            r = res[name]
            print(f"  {name:7s}: mean normal error {r['before']:.4f} -> {r['after']:.4f}, test PSNR {r['psnr']:.2f} dB")
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=600)
    ap.add_argument("--views", type=int, default=12)
    ap.add_argument("--size", type=int, default=96)
    ap.add_argument("--points", type=int, default=3000)
    ap.add_argument("--lam", type=float, default=0.05)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    r = run(a.iters, a.views, a.size, a.points, a.lam, a.out)
    assert r["normal"]["after"] < r["plain"]["after"], r
    assert all(math.isfinite(v) for run_ in r.values() for v in run_.values()), r


if __name__ == "__main__":
    main()
