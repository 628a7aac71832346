"""The cost of the filtered instantiations of k_project_fwd / k_project_bwd:
gs_project_forward and gs_project_backward (training configuration: raw scale
and rotation, DC colour, grad_sums given) of a bench config's scene (default
C3: 1M Gaussians, 1920x1080) through the C ABI, with the screen filter off,
on without compensation and on with it.  Each variant is timed with device
events around `--reps` back-to-back calls, the variants alternating over
`--rounds` rounds after a warm-up of every variant; the figure is the median
round's time per call, the spread the rounds' min..max.

    python tools/screen_filter_bench.py [config] [--reps 200] [--rounds 5]

Prints one JSON line (microseconds per call)."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

VARIANTS = (("off", 0.0, 0), ("plain", 0.3, 0), ("compensated", 0.3, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="C3")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as ge
    import bench
    pkg = ge.load_package()
    N, RZ = pkg._native, pkg.rasterizer
    lib = N.load()
    n, W, H = bench.CONFIGS[a.config]
    dev = torch.device("cuda", 0)
    sc = pkg.synthetic.make_scene(n, W, H, seed=0)
    m = pkg.synthetic.to_model(sc, pkg.GaussianModel, dev)

    class Cam:
        _width, _height, _FoVx, _FoVy = W, H, sc.fovx, sc.fovy
        world_view_transform = torch.eye(4)
    cam = pkg.camera_params(Cam(), pkg.RenderSettings(H, W, torch.zeros(3)))
    xyz, logits, opacity = m._xyz.detach(), m._features_dc.detach()[:, 0, :], m._opacity.detach()[:, 0]
    scaling, rotation = m._scaling.detach().contiguous(), m._rotation.detach().contiguous()
    gst = RZ._build_gaussians_struct(n, xyz, None, scaling, rotation, logits, opacity, True)
    f32, i32 = torch.float32, torch.int32
    E = lambda *shape, dtype=f32: torch.empty(shape, dtype=dtype, device=dev)
    means2d, conics, radii, vis = E(n, 2), E(n, 4), E(n), E(n, dtype=torch.uint8)
    records, rects, keys = E(n, N.GS_RECORD_FLOATS), E(n, 2, dtype=i32), E(n, dtype=i32)
    key_minmax = E(2 * ((n + 255) // 256), dtype=i32)
    gen = torch.Generator().manual_seed(1)
    grad_sums = (torch.rand((n, N.GS_PAIR_GRAD_FLOATS), generator=gen) * 2 - 1).to(dev)
    pair_offset = torch.zeros((n,), dtype=i32, device=dev)
    d_xyz, d_col, d_op, d_scl, d_rot = E(n, 3), E(n, 3), E(n), E(n, 3), E(n, 4)
    s = torch.cuda.current_stream().cuda_stream

    def args(variance, compensate):
        flt = N.GsScreenFilter(variance, compensate)
        pa = N.GsProjectArgs(cam.to_struct(), gst, N.ptr(means2d), N.ptr(conics), N.ptr(radii), N.ptr(vis),
                             N.ptr(records), N.ptr(rects), N.ptr(keys), 0, 32, N.ptr(key_minmax), flt)
        pb = N.GsProjectBwdArgs(cam.to_struct(), gst, N.ptr(means2d), N.ptr(conics), N.ptr(vis), N.ptr(rects),
                                N.ptr(pair_offset), None, None, None, None, N.ptr(d_xyz), None, N.ptr(d_scl),
                                N.ptr(d_rot), N.ptr(d_col), N.ptr(d_op), None, None, N.ptr(grad_sums), 0, flt)
        return pa, pb

    def timed(call, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            N.check(call(), "call")
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    res = {"config": a.config, "gaussians": n, "reps": a.reps, "rounds": a.rounds}
    calls = {}
    for name, variance, comp in VARIANTS:
        pa, pb = args(variance, comp)
        calls[name] = (pa, pb, lambda pa=pa: lib.gs_project_forward(C.byref(pa), s),
                       lambda pb=pb: lib.gs_project_backward(C.byref(pb), s))
    for which, idx in (("forward", 2), ("backward", 3)):
        times = {name: [] for name, _, _ in VARIANTS}
        for r in range(a.rounds + 1):  # round 0: the warm-up of every variant
            for name, _, _ in VARIANTS:
                if which == "backward":  # (the backward reads the forward's conics: its own variant's)
                    N.check(calls[name][2](), "forward")
                t = timed(calls[name][idx], a.reps)
                if r:
                    times[name].append(t)
        res[which + "_us"] = {k: round(statistics.median(v), 2) for k, v in times.items()}
        res[which + "_us_min_max"] = {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()}
    res["visible"] = int(vis.sum())
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
