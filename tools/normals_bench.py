"""The cost of the four normal-consistency kernels at N Gaussians (default 1M)
and a W x H image (default 1920 x 1080): gs_gaussian_normals_forward /
_backward and gs_normal_consistency_forward / _backward through the C ABI, and
in the same run the same maps composed from torch ops -- the alternative the
kernels replace (their backward through autograd, timed as forward + backward).
Each variant is timed with device events around `--reps` back-to-back calls,
the variants alternating over `--rounds` rounds after a warm-up of every
variant; the figure is the median round's time per call, the spread the rounds'
min..max.  Beside each kernel: the time its bytes need at the HBM peak (8.0 TB/s
spec, 6.29 TB/s measured for a float4 copy).  Under
`rocprofv3 --kernel-trace --stats` the four kernels' own times are those of
k_gaussian_normals_fwd / _bwd and k_normal_consistency_fwd / _bwd.

    python tools/normals_bench.py [--n 1000000] [--width 1920] [--height 1080] [--reps 200] [--rounds 5]

Prints one JSON line (microseconds per call)."""
import argparse
import ctypes as C
import json
import math
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_SPEC, HBM_COPY = 8.0e12, 6.29e12  # bytes / s


def torch_gaussian_normals(q, s, xyz, Rv, t):
    qh = q / q.norm(dim=1, keepdim=True).clamp_min(1e-12)
    w, x, y, z = qh.unbind(1)
    cols = torch.stack([
        torch.stack([1 - 2 * (y * y + z * z), 2 * (x * y + w * z), 2 * (x * z - w * y)], 1),
        torch.stack([2 * (x * y - w * z), 1 - 2 * (x * x + z * z), 2 * (y * z + w * x)], 1),
        torch.stack([2 * (x * z + w * y), 2 * (y * z - w * x), 1 - 2 * (x * x + y * y)], 1)], 1)  # [n, k, 3]
    k = s.argmin(1)
    nw = cols.gather(1, k.view(-1, 1, 1).expand(-1, 1, 3)).squeeze(1)
    nc = nw @ Rv.T
    pc = xyz @ Rv.T + t
    return torch.where(((nc * pc).sum(1) > 0).unsqueeze(1), -nc, nc)


def torch_consistency(Nr, D, A, r):
    P = D.unsqueeze(0) * r
    dx = P[:, 1:-1, 2:] - P[:, 1:-1, :-2]
    dy = P[:, 2:, 1:-1] - P[:, :-2, 1:-1]
    m = torch.cross(dx, dy, dim=0)
    ln = m.norm(dim=0, keepdim=True)
    nd = torch.where(ln > 1e-20, m / ln.clamp_min(1e-20), torch.zeros_like(m))
    nd = torch.nn.functional.pad(nd, (1, 1, 1, 1))
    return 1 - A * (Nr * nd).sum(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    N = pkg._native
    lib = N.load()
    n, W, H = a.n, a.width, a.height
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    R = lambda *shape: torch.rand(shape, generator=gen)
    q = (R(n, 4) * 2 - 1).to(dev)
    s = torch.log(0.005 + 0.05 * R(n, 3)).to(dev)
    xyz = (R(n, 3) * 4 - 2).to(dev)
    g_n = (R(n, 3) * 2 - 1).to(dev)
    view = [1.0, 0, 0, 0.1, 0, 1, 0, -0.2, 0, 0, 1, 4.0]
    Rv, t = torch.tensor(view).reshape(3, 4)[:, :3].to(dev), torch.tensor(view).reshape(3, 4)[:, 3].to(dev)
    normals, d_q = torch.empty(n, 3, device=dev), torch.empty(n, 4, device=dev)
    ga = N.GsGaussianNormalsArgs(n, q.data_ptr(), s.data_ptr(), xyz.data_ptr(), 3, (C.c_float * 12)(*view),
                                 normals.data_ptr(), g_n.data_ptr(), d_q.data_ptr())
    fx = fy = 0.5 * W / math.tan(0.5)
    Nr = (R(3, H, W) * 2 - 1).to(dev)
    D = (3 + 0.5 * R(H, W)).to(dev)
    A, g_e = R(H, W).to(dev), (R(H, W) * 2 - 1).to(dev)
    err, nd = torch.empty(H, W, device=dev), torch.empty(3, H, W, device=dev)
    d_n, d_d = torch.empty(3, H, W, device=dev), torch.empty(H, W, device=dev)
    ca = N.GsNormalConsistencyArgs(W, H, fx, fy, W * 0.5, H * 0.5, Nr.data_ptr(), D.data_ptr(), A.data_ptr(),
                                   err.data_ptr(), None, g_e.data_ptr(), d_n.data_ptr(), d_d.data_ptr())
    yy, xx = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                            torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    rays = torch.stack([(xx - W * 0.5) / fx, -(yy - H * 0.5) / fy, torch.ones_like(xx)])
    stream = torch.cuda.current_stream().cuda_stream
    q_g, Nr_g, D_g = q.clone().requires_grad_(True), Nr.clone().requires_grad_(True), D.clone().requires_grad_(True)

    def gn_fwdbwd_torch():
        torch.autograd.grad(torch_gaussian_normals(q_g, s, xyz, Rv, t), q_g, g_n)

    def nc_fwdbwd_torch():
        torch.autograd.grad(torch_consistency(Nr_g, D_g, A, rays), (Nr_g, D_g), g_e)

    def no_grad(f, *args):
        with torch.no_grad():
            return f(*args)
    variants = {
        "gaussian_normals_forward": lambda: N.check(lib.gs_gaussian_normals_forward(C.byref(ga), stream), "gn fwd"),
        "gaussian_normals_backward": lambda: N.check(lib.gs_gaussian_normals_backward(C.byref(ga), stream), "gn bwd"),
        "normal_consistency_forward": lambda: N.check(lib.gs_normal_consistency_forward(C.byref(ca), stream), "nc fwd"),
        "normal_consistency_backward": lambda: N.check(lib.gs_normal_consistency_backward(C.byref(ca), stream), "nc bwd"),
        "gaussian_normals_forward_torch": lambda: no_grad(torch_gaussian_normals, q, s, xyz, Rv, t),
        "gaussian_normals_forward_backward_torch": gn_fwdbwd_torch,
        "normal_consistency_forward_torch": lambda: no_grad(torch_consistency, Nr, D, A, rays),
        "normal_consistency_forward_backward_torch": nc_fwdbwd_torch,
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
    # the torch maps say what the kernels say (fp32 against fp32)
    lib.gs_gaussian_normals_forward(C.byref(ga), stream)
    lib.gs_normal_consistency_forward(C.byref(ca), stream)
    with torch.no_grad():
        agree = {"normals": float((torch_gaussian_normals(q, s, xyz, Rv, t) - normals).abs().max()),
                 "error": float((torch_consistency(Nr, D, A, rays) - err).abs().max())}
    px = W * H
    bytes_ = {"gaussian_normals_forward": 52 * n, "gaussian_normals_backward": 68 * n,
              "normal_consistency_forward": 24 * px, "normal_consistency_backward": 40 * px}
    res = {"gaussians": n, "width": W, "height": H, "reps": a.reps, "rounds": a.rounds,
           "us": {k: round(statistics.median(v), 2) for k, v in times.items()},
           "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
           "bytes": bytes_,
           "hbm_us_at_8.0TBs": {k: round(b / HBM_SPEC * 1e6, 2) for k, b in bytes_.items()},
           "hbm_us_at_6.29TBs": {k: round(b / HBM_COPY * 1e6, 2) for k, b in bytes_.items()},
           "torch_minus_kernel": agree}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
