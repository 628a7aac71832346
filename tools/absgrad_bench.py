"""Frames for a kernel trace of the absolute-gradient path next to the product
one: a bench config's scene (default C3: 1M Gaussians, 1920x1080), rendered
forward + backward through GaussianRenderer.render, random cotangents on image
/ alpha / depth -- `--reps` frames with DensityStats(abs_grad=True) (the stage
path: k_blend_bwd<..., kAbs>, k_gather_abs, k_density_accumulate_abs) and
`--reps` with plain DensityStats (the product k_blend_bwd, k_gather_slots,
k_density_accumulate).  The timing is the trace's, taken in a run of its own:
    rocprofv3 --kernel-trace --stats -d <dir> -o run --output-format csv -- \\
        python tools/absgrad_bench.py [config] [--reps 10]
then the kernels side by side in <dir>/*kernel_stats.csv (the two k_blend_bwd
instantiations differ in their third template argument).
Prints one JSON line: the Gaussians, how many the view saw, the frames run per
path, the largest relative difference of the two paths' signed statistics (0:
the same bits) and the ratio of the mean absolute to the mean signed statistic."""
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
    ap.add_argument("--reps", type=int, default=10)
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
    frames = 3 + a.reps
    both = (pkg.DensityStats(n, dev, abs_grad=True), pkg.DensityStats(n, dev))
    for stats in both:
        for _ in range(frames):
            for p in m.parameters():
                p.grad = None
            out = r.render(cam, m, st, density_stats=stats)
            ((out["image"] * gi).sum() + (out["alpha"] * ga).sum() + (out["depth"] * gd).sum()).backward()
    torch.cuda.synchronize()
    s_abs, s_plain = both
    seen = s_abs.denom > 0
    assert float(s_abs.denom.max()) == frames == float(s_plain.denom.max())
    diff = float(((s_abs.grad_accum - s_plain.grad_accum).abs() / s_plain.grad_accum.clamp_min(1e-30))[seen].max())
    print(json.dumps({"config": a.config, "gaussians": n, "visible": int(seen.sum()), "frames_per_path": frames,
                      "signed_statistic_max_rel_diff": diff,
                      "mean_abs_over_signed": float(s_abs.mean_abs_grad()[seen].mean() / s_abs.mean_grad()[seen].mean())}),
          flush=True)


if __name__ == "__main__":
    main()
