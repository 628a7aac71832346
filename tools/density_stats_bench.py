"""Frames for a kernel trace of gs_density_accumulate next to the projection
backward it follows: a bench config's scene (default C3: 1M Gaussians,
1920x1080), rendered forward + backward through GaussianRenderer.render with
density_stats, random cotangents on image / alpha / depth.  The timing is the
trace's, taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o run --output-format csv -- \\
        python tools/density_stats_bench.py [config] [--reps 20]
then k_density_accumulate beside k_project_bwd in <dir>/*kernel_stats.csv.
Prints one JSON line: the Gaussians, how many the view saw, the frames run,
and the kernel's bytes from shapes (1 B vis per Gaussian; per visible one the
40 B grad_sums row whose cache lines move whole, 4 B radius, 24 B of
statistics read and written)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="C3")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    import __graft_entry__ as ge
    import bench
    from stubs import Cam
    pkg = ge.load_package()
    n, W, H = bench.CONFIGS[a.config]
    dev = torch.device("cuda", 0)
    sc = pkg.synthetic.make_scene(n, W, H, seed=0)
    m = pkg.synthetic.to_model(sc, pkg.GaussianModel, dev)
    cam, st = Cam(W, H, sc.fovx, sc.fovy), pkg.RenderSettings(H, W, torch.zeros(3))
    g = torch.Generator().manual_seed(1)
    gi, ga, gd = [(torch.rand(s, generator=g) * 2 - 1).to(dev) for s in ((3, H, W), (1, H, W), (1, H, W))]
    r = pkg.GaussianRenderer()
    stats = m.density_stats
    for _ in range(3 + a.reps):
        for p in m.parameters():
            p.grad = None
        out = r.render(cam, m, st, density_stats=stats)
        ((out["image"] * gi).sum() + (out["alpha"] * ga).sum() + (out["depth"] * gd).sum()).backward()
    torch.cuda.synchronize()
    seen = int((stats.denom > 0).sum())
    assert float(stats.denom.max()) == 3 + a.reps
    print(json.dumps({"config": a.config, "gaussians": n, "visible": seen, "frames": 3 + a.reps,
                      "bytes_per_launch": n + seen * (40 + 4 + 24)}), flush=True)


if __name__ == "__main__":
    main()
