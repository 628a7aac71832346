"""What densify_criterion = "mcmc" adds to a training step, at a bench config's
scene (default C3: 1M Gaussians, 1920x1080): device-event time of
gs_mcmc_noise and gs_mcmc_regularize (the two per-iteration launches) beside
their algorithmic bytes, and of one GaussianModel.relocate_and_grow with 5 % of
the Gaussians dead -- in place at the cap, and growing by 5 %.  The clocks are
brought up first by the spin-up the bench uses (50 untimed render + backward +
Adam steps at C3).
    python tools/mcmc_step_bench.py [config] [--reps 200] [--spinup-steps 50] [--step-ms MS]
--step-ms: the ms_per_step of a bench.py line taken on the same box; the
launches are then also printed as shares of it.  Prints one JSON line."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

NOISE_BYTES = 56       # per Gaussian: xyz 12, scaling 12, rotation 16, opacity 4 read; xyz 12 written
REGULARIZE_BYTES = 48  # per Gaussian: opacity 4 and scaling 12 read; 16 B of gradients read and written again


def _timed(fn, reps):
    """Mean device-event microseconds of fn() over `reps` back-to-back calls."""
    for _ in range(5):
        fn()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / reps


def _refine(pkg, m, opt, cap, seed):
    """One relocate_and_grow with every 20th Gaussian dead: (ms, info)."""
    with torch.no_grad():
        m._opacity[::20] = -8.0
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    t0.record()
    info = m.relocate_and_grow(cap, 0.005, seed, optimizer=opt)
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1), info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="C3")
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--spinup-steps", type=int, default=50)
    ap.add_argument("--step-ms", type=float, default=None)
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
    opt = pkg.optim.FusedAdam([{"params": [p], "lr": 1e-6} for p in m.parameter_list()])
    r = pkg.GaussianRenderer()
    target = torch.rand(3, H, W, generator=torch.Generator().manual_seed(1)).to(dev)
    for _ in range(a.spinup_steps):
        opt.zero_grad()
        pkg.photometric_loss(r.render(cam, m, st)["image"], target, 0.2)[0].backward()
        opt.step()
    torch.cuda.synchronize()
    d_op, d_sc = torch.zeros_like(m._opacity), torch.zeros_like(m._scaling)
    xyz = m._xyz.detach().clone()
    noise_us = _timed(lambda: pkg.mcmc_noise(xyz, m._scaling.data, m._rotation.data, m._opacity.data, 1e-3, 7), a.reps)
    reg_us = _timed(lambda: pkg.mcmc_regularize(m._opacity.data, m._scaling.data, d_op, d_sc, 0.01, 0.01), a.reps)
    _refine(pkg, m, opt, n, 1)  # (untimed: code objects, allocator)
    place_ms, place = _refine(pkg, m, opt, n, 3)
    grow_ms, grow = _refine(pkg, m, opt, int(1.05 * n), 5)
    out = {"config": a.config, "gaussians": n, "reps": a.reps, "spinup_steps": a.spinup_steps,
           "noise_us": round(noise_us, 2), "noise_bytes": NOISE_BYTES * n,
           "noise_gb_s": round(NOISE_BYTES * n / noise_us / 1e3, 1),
           "regularize_us": round(reg_us, 2), "regularize_bytes": REGULARIZE_BYTES * n,
           "regularize_gb_s": round(REGULARIZE_BYTES * n / reg_us / 1e3, 1),
           "relocate_in_place_ms": round(place_ms, 3), "relocate_in_place": place,
           "relocate_and_grow_ms": round(grow_ms, 3), "relocate_and_grow": grow}
    if a.step_ms:
        out["step_ms"] = a.step_ms
        out["noise_share_of_step"] = round(noise_us / 1e3 / a.step_ms, 5)
        out["regularize_share_of_step"] = round(reg_us / 1e3 / a.step_ms, 5)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
