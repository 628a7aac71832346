"""The cost of the bilateral-grid kernels at a W x H image (default 1920 x 1080)
and a (Gw, Gh, L) grid (default 16 x 16 x 8): gs_bilagrid_slice_forward,
gs_bilagrid_slice_backward (two launches: d_rgb per pixel, d_grid as a gather)
and gs_bilagrid_tv through the C ABI, and in the same run the same slice
composed from torch ops -- 5-D grid_sample (bilinear, border, align_corners)
and the affine apply, its backward through autograd (float atomics into the
grid), timed as forward alone and forward + backward.  Each variant is timed
with device events around `--reps` back-to-back calls, the variants alternating
over `--rounds` rounds after a warm-up of every variant; the figure is the
median round's time per call, the spread the rounds' min..max.  Beside each
kernel: the time its image bytes need at the HBM peak (8.0 TB/s spec, 6.29 TB/s
measured for a float4 copy).  Under `rocprofv3 --kernel-trace --stats` the
kernels' own times are those of k_bilagrid_slice_fwd, k_bilagrid_slice_bwd_rgb,
k_bilagrid_slice_bwd_grid and k_bilagrid_tv.  Also reports whether two torch
backward passes give the same grid gradient bits, and the kernels'.

    python tools/bilagrid_bench.py [--width 1920] [--height 1080] [--grid 16 16 8] [--reps 200] [--rounds 5] [--random]

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

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12  # bytes / s


def torch_slice(G, rgb, uv):
    """grid_sample's slice and the apply; uv [H, W, 2] the constant (x, y) coordinates in [-1, 1]."""
    H, W = rgb.shape[1:]
    gray = 0.299 * rgb[0] + 0.587 * rgb[1] + 0.114 * rgb[2]
    coords = torch.cat([uv, (gray * 2 - 1).unsqueeze(-1)], -1)[None, None]
    A = torch.nn.functional.grid_sample(G[None], coords, mode="bilinear", padding_mode="border",
                                        align_corners=True).reshape(3, 4, H, W)
    return (A[:, :3] * rgb[None]).sum(1) + A[:, 3]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--grid", type=int, nargs=3, default=[16, 16, 8], metavar=("GW", "GH", "L"))
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--random", action="store_true", help="uniformly random colours instead of the smooth image")
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    N = pkg._native
    lib = N.load()
    W, H = a.width, a.height
    gw, gh, gl = a.grid
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    R = lambda *shape: torch.rand(shape, generator=gen)
    G = (pkg.bilagrid.identity_grid((gw, gh, gl)) + 0.3 * (R(12, gl, gh, gw) * 2 - 1)).to(dev)
    # a smooth image (neighbouring pixels on neighbouring gray levels, as in a photograph) plus noise
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    rgb = torch.stack([0.5 + 0.5 * torch.sin(6 * xx + 3 * yy), 0.5 + 0.5 * torch.cos(5 * yy - 2 * xx), xx * yy])
    rgb = (rgb * 1.1 - 0.05 + 0.02 * (R(3, H, W) * 2 - 1)).to(dev).contiguous()
    if a.random:  # (every pixel on its own gray level: the slice's worst case)
        rgb = (R(3, H, W) * 1.2 - 0.1).to(dev)
    g_out = (R(3, H, W) * 2 - 1).to(dev)
    out, d_rgb, d_grid = torch.empty_like(rgb), torch.empty_like(rgb), torch.empty_like(G)
    tv, d_tv = torch.empty((), device=dev), torch.empty_like(G)
    sa = N.GsBilagridSliceArgs(W, H, gw, gh, gl, G.data_ptr(), rgb.data_ptr(), out.data_ptr(), g_out.data_ptr(),
                               d_rgb.data_ptr(), d_grid.data_ptr())
    ta = N.GsBilagridTvArgs(gw, gh, gl, G.data_ptr(), tv.data_ptr(), d_tv.data_ptr())
    u = ((torch.arange(W, dtype=torch.float32) + 0.5) / W * 2 - 1).expand(H, W)
    v = ((torch.arange(H, dtype=torch.float32) + 0.5) / H * 2 - 1)[:, None].expand(H, W)
    uv = torch.stack([u, v], -1).to(dev).contiguous()
    stream = torch.cuda.current_stream().cuda_stream
    G_g, rgb_g = G.clone().requires_grad_(True), rgb.clone().requires_grad_(True)

    def fwd_torch():
        with torch.no_grad():
            return torch_slice(G, rgb, uv)

    def fwdbwd_torch():
        return torch.autograd.grad(torch_slice(G_g, rgb_g, uv), (G_g, rgb_g), g_out)

    def fwdbwd_hip():
        N.check(lib.gs_bilagrid_slice_forward(C.byref(sa), stream), "slice fwd")
        N.check(lib.gs_bilagrid_slice_backward(C.byref(sa), stream), "slice bwd")
    variants = {
        "slice_forward": lambda: N.check(lib.gs_bilagrid_slice_forward(C.byref(sa), stream), "slice fwd"),
        "slice_backward": lambda: N.check(lib.gs_bilagrid_slice_backward(C.byref(sa), stream), "slice bwd"),
        "slice_forward_backward": fwdbwd_hip,
        "tv": lambda: N.check(lib.gs_bilagrid_tv(C.byref(ta), stream), "tv"),
        "slice_forward_torch": fwd_torch,
        "slice_forward_backward_torch": fwdbwd_torch,
    }

    def timed(call, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    times = {k: [] for k in variants}
    for r in range(a.rounds + 1):  # round 0: the warm-up of every variant
        for name, call in variants.items():
            tm = timed(call, a.reps if not name.endswith("torch") else max(1, a.reps // 10))
            if r:
                times[name].append(tm)
    # the torch composition says what the kernels say (fp32 against fp32), and who repeats its bits
    fwdbwd_hip()
    first = d_grid.clone()
    fwdbwd_hip()
    t_grid, t_rgb = fwdbwd_torch()
    t_grid2, _ = fwdbwd_torch()
    torch.cuda.synchronize()
    agree = {"out": float((fwd_torch() - out).abs().max()), "d_rgb": float((t_rgb - d_rgb).abs().max()),
             "d_grid_of_max": float((t_grid - d_grid).abs().max() / d_grid.abs().max())}
    repeat = {"kernel_d_grid_same_bits": bool(torch.equal(first.view(torch.int32), d_grid.view(torch.int32))),
              "torch_d_grid_same_bits": bool(torch.equal(t_grid.view(torch.int32), t_grid2.view(torch.int32)))}
    px = W * H
    bytes_ = {"slice_forward": 24 * px, "slice_backward": 36 * px + 24 * px + 4 * G.numel(), "tv": 8 * G.numel()}
    bytes_["slice_forward_backward"] = bytes_["slice_forward"] + bytes_["slice_backward"]
    res = {"width": W, "height": H, "grid": [gw, gh, gl], "image": "random" if a.random else "smooth", "reps": a.reps, "rounds": a.rounds,
           "us": {k: round(statistics.median(v), 2) for k, v in times.items()},
           "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
           "bytes": bytes_,
           "hbm_us_at_8.0TBs": {k: round(b / HBM_SPEC * 1e6, 2) for k, b in bytes_.items()},
           "hbm_us_at_6.29TBs": {k: round(b / HBM_COPY * 1e6, 2) for k, b in bytes_.items()},
           "torch_minus_kernel": agree, "repeat": repeat}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
