"""Cost of the two depth-distortion kernels next to the colour blend and a
one-chunk feature pass of the same frame.

On one frame of a bench config (default C3: 1M Gaussians, 1920x1080, tile 16)
this times, with StageTimer marks on the render stream and from one build,
  * gs_blend_forward and gs_blend_backward (the colour pass, unchanged);
  * gs_blend_features_forward and gs_blend_features_backward with C = 4 (one
    chunk), the kernels the distortion pair was modelled on;
  * gs_blend_distortion_forward and gs_blend_distortion_backward, with the
    linear and with the inverse depth map;
  * the two gathers behind the backwards (gs_gather_feature_partials,
    gs_gather_partials with accumulate = 1), each on its own.
Every item is the launch alone (flag clears and gathers are timed apart).
The GPU is spun up first (the clock ramps over the first ~60 ms of load), then
5 warm-up and 20 timed repetitions per item; medians.  One JSON line: times in
ms, and the distortion kernels over their feature counterparts.

usage: python tools/distortion_bench.py [config] [--reps 20]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def staged(RZ, fn, name, reps, warmup=5):
    """Median ms of fn()'s launches between two StageTimer marks."""
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    RZ.StageTimer.enabled, RZ.StageTimer.only = True, None
    RZ.StageTimer.reset()
    for _ in range(reps):
        RZ.StageTimer.mark(name)
        fn()
        RZ.StageTimer.mark("~end_" + name)
    d = RZ.StageTimer.durations_ms()
    RZ.StageTimer.enabled = False
    RZ.StageTimer.reset()
    return round(statistics.median(d[name]), 4)


def run(config="C3", reps=20, seed=0, near_far=(0.1, 1000.0)):
    import __graft_entry__ as ge
    import bench
    pkg = ge.load_package()
    N = pkg._native
    from mini3dgs_amd import rasterizer as RZ
    from stubs import Cam
    n, W, H = bench.CONFIGS[config]
    dev = torch.device("cuda", 0)
    sc = pkg.synthetic.make_scene(n, W, H, seed=seed)
    m = pkg.synthetic.to_model(sc, pkg.GaussianModel, dev)
    camp = pkg.camera_params(Cam(W, H, sc.fovx, sc.fovy), pkg.RenderSettings(H, W, torch.zeros(3)))
    cs = camp.to_struct()
    g = torch.Generator().manual_seed(1)
    gi, ga, gd = [(torch.rand(s, generator=g) * 2 - 1).to(dev) for s in ((3, H, W), (1, H, W), (1, H, W))]
    lib = N.load()
    with torch.no_grad():
        out = RZ.forward_pipeline(camp, m._xyz, None, m._scaling, m._rotation, m._features_dc, m._opacity,
                                  opacity_is_logit=True, need_grad=True, stage_path=True)
    image, alpha, depth = out[:3]
    fr = out[7]
    T, G = fr.T, fr.groups
    live = fr.live_bits
    lw = 0 if live is None else live.shape[1]
    s = N.stream_ptr()
    f32 = torch.float32
    frame = (cs, camp.tiles_x, camp.tiles_y, N.ptr(fr.ranges), N.ptr(fr.sorted_gauss), N.ptr(fr.records))
    replay = RZ.replay_frame(camp, fr, n)

    # the colour pass, the forward into scratch copies of everything it writes
    scratch = [torch.empty_like(t) for t in (image, alpha, depth, fr.pix_flags, fr.cell_neval)]
    live2 = None if live is None else torch.empty_like(live)
    cf = N.GsBlendFwdArgs(*frame, *(N.ptr(t) for t in scratch), N.ptr(live2), lw, None, T, None)
    pg = torch.empty((T * G, N.GS_PARTIAL_STRIDE), dtype=f32, device=dev)
    flags = torch.zeros((T * G,), dtype=torch.uint8, device=dev)
    sums = torch.zeros((n, N.GS_PAIR_GRAD_FLOATS), dtype=f32, device=dev)
    cb = N.GsBlendBwdArgs(*frame, N.ptr(image), N.ptr(alpha), N.ptr(depth), N.ptr(fr.pix_flags), N.ptr(fr.cell_neval),
                          N.ptr(gi), N.ptr(ga), N.ptr(gd), N.ptr(live), lw, N.ptr(pg), N.ptr(flags), T, 0, 0)
    cg = N.GsProjectBwdArgs()
    cg.g.n = n
    cg.vis, cg.rects, cg.pair_offset = N.ptr(fr.vis), N.ptr(fr.rects), N.ptr(fr.pair_offset)
    cg.pair_grads, cg.slot_live, cg.grad_sums, cg.partial_groups = N.ptr(pg), N.ptr(flags), N.ptr(sums), G

    # one feature chunk
    F = torch.rand((n, 4), generator=g).to(dev)
    stagedF = RZ._stage_features(F)
    fimg = torch.empty((4, H, W), dtype=f32, device=dev)
    gF = (torch.rand((4, H, W), generator=g) * 2 - 1).to(dev)
    dF = torch.empty((n, 4), dtype=f32, device=dev)
    ff = N.GsFeatureFwdArgs(replay, 4, N.ptr(stagedF), N.ptr(fimg))
    fb = N.GsFeatureBwdArgs(replay, 4, 0, N.ptr(stagedF), N.ptr(fimg), N.ptr(gF), N.ptr(pg), N.ptr(flags), 0, 0)
    fg = N.GsFeatureGatherArgs(n, N.ptr(fr.vis), N.ptr(fr.rects), N.ptr(fr.pair_offset), N.ptr(pg), N.ptr(flags),
                               G, 1, N.ptr(sums), N.ptr(dF), dF.stride(0), 0, 4, 0)

    # the distortion pass
    dist = torch.empty((H, W), dtype=f32, device=dev)
    mom = torch.empty((2, H, W), dtype=f32, device=dev)
    medz = torch.empty((H, W), dtype=f32, device=dev)
    medi = torch.empty((H, W), dtype=torch.int32, device=dev)
    gD = (torch.rand((H, W), generator=g) * 2 - 1).to(dev)
    df = N.GsDistortionFwdArgs(replay, 0.0, 0.0, N.ptr(dist), N.ptr(mom), N.ptr(medz), N.ptr(medi))
    db = N.GsDistortionBwdArgs(replay, 0.0, 0.0, N.ptr(dist), N.ptr(mom), N.ptr(gD), N.ptr(pg), N.ptr(flags), 0, 0)

    def call(fn, args, what, *extra):
        return lambda: N.check(fn(C.byref(args), *extra, s), what)
    colour_fwd = call(lib.gs_blend_forward, cf, "gs_blend_forward")
    colour_bwd = call(lib.gs_blend_backward, cb, "gs_blend_backward")
    feat_fwd = call(lib.gs_blend_features_forward, ff, "gs_blend_features_forward")
    feat_bwd = call(lib.gs_blend_features_backward, fb, "gs_blend_features_backward")
    feat_gather = call(lib.gs_gather_feature_partials, fg, "gs_gather_feature_partials")
    dist_fwd = call(lib.gs_blend_distortion_forward, df, "gs_blend_distortion_forward")
    dist_bwd = call(lib.gs_blend_distortion_backward, db, "gs_blend_distortion_backward")
    gather = call(lib.gs_gather_partials, cg, "gs_gather_partials", 1)

    # spin-up: ~100 ms of the heaviest launch before anything is timed (every
    # replayed slot's flag is set again by each backward: no clear in a timed region)
    for _ in range(120):
        colour_bwd()
    torch.cuda.synchronize()
    t = lambda fn, name: staged(RZ, fn, name, reps)
    res = {"config": config, "n": n, "width": W, "height": H, "tile": camp.tile_size, "entries": T, "reps": reps,
           "device": torch.cuda.get_device_name(0),
           "colour_fwd_ms": t(colour_fwd, "colour_fwd"), "colour_bwd_ms": t(colour_bwd, "colour_bwd")}
    feat_fwd()  # (the backward reads the forward's image)
    res["feature_fwd_ms"], res["feature_bwd_ms"] = t(feat_fwd, "feature_fwd"), t(feat_bwd, "feature_bwd")
    res["feature_gather_ms"] = t(feat_gather, "feature_gather")
    for label, (near, far) in (("linear", (0.0, 0.0)), ("inverse", near_far)):
        df.near = db.near = near
        df.far = db.far = far
        dist_fwd()
        fw, bw = t(dist_fwd, "distortion_fwd"), t(dist_bwd, "distortion_bwd")
        res[label] = {"mean_distortion": float(dist.mean()), "distortion_fwd_ms": fw, "distortion_bwd_ms": bw,
                      "fwd_over_feature_fwd": round(fw / res["feature_fwd_ms"], 3),
                      "bwd_over_feature_bwd": round(bw / res["feature_bwd_ms"], 3),
                      "fwd_over_colour_fwd": round(fw / res["colour_fwd_ms"], 3),
                      "bwd_over_colour_bwd": round(bw / res["colour_bwd_ms"], 3)}
    res["gather_accumulate_ms"] = t(gather, "gather")
    torch.cuda.synchronize()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", nargs="?", default="C3")
    ap.add_argument("--reps", type=int, default=20)
    a = ap.parse_args()
    print(json.dumps(run(a.config, a.reps)))


if __name__ == "__main__":
    main()
