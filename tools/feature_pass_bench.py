"""Cost of the feature pass next to the colour pass of the same frame.

On one frame of a bench config (default C3: 1M Gaussians, 1920x1080, tile 16)
this times, with HIP events on the render stream,
  * gs_blend_forward (k_blend_fwd) and gs_blend_backward + gs_gather_partials
    (k_blend_bwd + k_gather_slots): the yardstick, unchanged kernels;
  * gs_blend_features_forward, and per chunk gs_blend_features_backward +
    gs_gather_feature_partials with the flag clear between them (what
    rasterizer._feature_backward launches), for C = 4 and C = 16.
The GPU is spun up first (the clock ramps over the first ~60 ms of load), then
5 warm-up and 20 timed repetitions per item; the median is reported.  One
JSON line: times in ms, and each feature item per chunk over its colour
counterpart ("about one colour pass per chunk" is the expectation: a chunk
walks the same entries with the same payload width).

usage: python tools/feature_pass_bench.py [config] [--reps 20]"""
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


def timed(fn, reps, warmup=5):
    """Median ms of fn()'s launches over `reps` repetitions (HIP events)."""
    for _ in range(warmup):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return statistics.median(ms)


def run(config="C3", reps=20, channels=(4, 16), seed=0):
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

    # the colour forward again, into scratch copies of everything it writes
    scratch = [torch.empty_like(t) for t in (image, alpha, depth, fr.pix_flags, fr.cell_neval)]
    live2 = None if live is None else torch.empty_like(live)
    cf = N.GsBlendFwdArgs(cs, camp.tiles_x, camp.tiles_y, N.ptr(fr.ranges), N.ptr(fr.sorted_gauss), N.ptr(fr.records),
                          *(N.ptr(t) for t in scratch), N.ptr(live2), lw, None, T, None)
    pg = torch.empty((T * G, N.GS_PARTIAL_STRIDE), dtype=f32, device=dev)
    flags = torch.zeros((T * G,), dtype=torch.uint8, device=dev)
    sums = torch.empty((n, N.GS_PAIR_GRAD_FLOATS), dtype=f32, device=dev)
    cb = N.GsBlendBwdArgs(cs, camp.tiles_x, camp.tiles_y, N.ptr(fr.ranges), N.ptr(fr.sorted_gauss), N.ptr(fr.records),
                          N.ptr(image), N.ptr(alpha), N.ptr(depth), N.ptr(fr.pix_flags), N.ptr(fr.cell_neval),
                          N.ptr(gi), N.ptr(ga), N.ptr(gd), N.ptr(live), lw, N.ptr(pg), N.ptr(flags), T, 0, 0)
    cg = N.GsProjectBwdArgs()
    cg.g.n = n
    cg.vis, cg.rects, cg.pair_offset = N.ptr(fr.vis), N.ptr(fr.rects), N.ptr(fr.pair_offset)
    cg.pair_grads, cg.slot_live, cg.grad_sums, cg.partial_groups = N.ptr(pg), N.ptr(flags), N.ptr(sums), G

    def colour_fwd():
        N.check(lib.gs_blend_forward(C.byref(cf), s), "gs_blend_forward")

    def colour_bwd():
        # (every replayed slot's flag is set again by each repetition: the flags
        # stay as the first one left them, no clear in the timed region -- in the
        # render the forward's gs_tile_ranges clears them)
        N.check(lib.gs_blend_backward(C.byref(cb), s), "gs_blend_backward")
        N.check(lib.gs_gather_partials(C.byref(cg), 0, s), "gs_gather_partials")

    # spin-up: ~100 ms of the heaviest launch before anything is timed
    for _ in range(120):
        colour_bwd()
    torch.cuda.synchronize()
    res = {"config": config, "n": n, "width": W, "height": H, "tile": camp.tile_size, "entries": T, "reps": reps,
           "device": torch.cuda.get_device_name(0),
           "colour_fwd_ms": round(timed(colour_fwd, reps), 4), "colour_bwd_gather_ms": round(timed(colour_bwd, reps), 4)}
    for c in channels:
        F = torch.rand((n, c), generator=g).to(dev)
        staged = RZ._stage_features(F)
        fimg = torch.empty((c, H, W), dtype=f32, device=dev)
        gF = (torch.rand((c, H, W), generator=g) * 2 - 1).to(dev)
        dF = torch.empty((n, c), dtype=f32, device=dev)
        replay = RZ.replay_frame(camp, fr, n)
        ff = N.GsFeatureFwdArgs(replay, c, N.ptr(staged), N.ptr(fimg))
        fb = N.GsFeatureBwdArgs(replay, c, 0, N.ptr(staged), N.ptr(fimg), N.ptr(gF), N.ptr(pg), N.ptr(flags), 0, 0)
        fg = N.GsFeatureGatherArgs(n, N.ptr(fr.vis), N.ptr(fr.rects), N.ptr(fr.pair_offset), N.ptr(pg), N.ptr(flags),
                                   G, 1, N.ptr(sums), N.ptr(dF), dF.stride(0), 0, 0, 0)
        chunks = (c + N.GS_FEATURE_CHUNK - 1) // N.GS_FEATURE_CHUNK

        def feat_fwd():
            N.check(lib.gs_blend_features_forward(C.byref(ff), s), "gs_blend_features_forward")

        def feat_bwd():
            for k in range(chunks):
                fb.chunk, fg.channel_begin = k, k * N.GS_FEATURE_CHUNK
                fg.channel_count = min(N.GS_FEATURE_CHUNK, c - fg.channel_begin)
                flags.zero_()
                N.check(lib.gs_blend_features_backward(C.byref(fb), s), "gs_blend_features_backward")
                N.check(lib.gs_gather_feature_partials(C.byref(fg), s), "gs_gather_feature_partials")

        feat_fwd()  # (the backward reads the forward's image)
        fw, bw = timed(feat_fwd, reps), timed(feat_bwd, reps)
        res[f"C{c}"] = {"chunks": chunks, "fwd_ms": round(fw, 4), "bwd_gather_ms": round(bw, 4),
                        "fwd_per_chunk_over_colour_fwd": round(fw / chunks / res["colour_fwd_ms"], 3),
                        "bwd_per_chunk_over_colour_bwd": round(bw / chunks / res["colour_bwd_gather_ms"], 3)}
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
