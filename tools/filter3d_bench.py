"""The cost of the 3D smoothing filter's three kernels at N Gaussians (default
1M): gs_filter3d_forward, gs_filter3d_backward and gs_filter3d_accumulate over
K cameras (default 100) through the C ABI, and in the same run the same maps
written in torch ops -- the alternative the kernels replace.  Each variant is
timed with device events around `--reps` back-to-back calls, the variants
alternating over `--rounds` rounds after a warm-up of every variant; the
figure is the median round's time per call, the spread the rounds' min..max.
Beside each kernel: the time its bytes need at the HBM peak (8.0 TB/s spec,
6.29 TB/s measured for a float4 copy).

    python tools/filter3d_bench.py [--n 1000000] [--cameras 100] [--reps 200] [--rounds 5]

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


def torch_forward(s, o, f):
    L = torch.log(f).unsqueeze(1)
    d = 2.0 * (s - L)
    s_out = torch.maximum(s, L) + 0.5 * torch.log1p(torch.exp(-d.abs()))
    on = (f > 0).unsqueeze(1)
    return torch.where(on, s_out, s), torch.sigmoid(o) * torch.where(on[:, 0], torch.sigmoid(d).prod(1).sqrt(), 1.0)


def torch_backward(s, o, f, g_s, g_o):
    d = 2.0 * (s - torch.log(f).unsqueeze(1))
    on = (f > 0).unsqueeze(1)
    r, q = torch.where(on, torch.sigmoid(d), 1.0), torch.where(on, torch.sigmoid(-d), 0.0)
    coef, so = r.prod(1).sqrt(), torch.sigmoid(o)
    return g_s * r + (g_o * so * coef).unsqueeze(1) * q, g_o * coef * so * (1 - so)


def torch_rate(xyz, cams, near, margin, max_rate, chunk=10):
    """fp32 (the kernel decides in fp64), `chunk` cameras at a time ([n, chunk] temporaries)."""
    for c in cams.split(chunk):
        v = c[:, :12].reshape(-1, 3, 4)
        p = torch.einsum("kij,nj->nki", v[:, :, :3], xyz) + v[:, :, 3]
        X, Y, Z = p.unbind(-1)
        fx, fy, cx, cy, W, H = c[:, 12:].unbind(1)
        u, w = fx * X / Z + cx, fy * Y / Z + cy
        ok = (Z > near) & (u >= -margin * W) & (u <= (1 + margin) * W) & (w >= -margin * H) & (w <= (1 + margin) * H)
        rate = torch.where(ok, torch.maximum(fx, fy) / Z, 0.0).amax(1)
        torch.maximum(max_rate, rate, out=max_rate)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--cameras", type=int, default=100)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    N = pkg._native
    lib = N.load()
    n, K = a.n, a.cameras
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(0)
    R = lambda *shape: torch.rand(shape, generator=gen)
    xyz = (R(n, 3) * 4 - 2).to(dev)
    s = torch.log(0.005 + 0.05 * R(n, 3)).to(dev)
    o = (R(n) * 8 - 4).to(dev)
    g_s, g_o = (R(n, 3) * 2 - 1).to(dev), (R(n) * 2 - 1).to(dev)
    rows = []
    for k in range(K):  # a ring of cameras at radius 4 looking at the origin
        th = 2 * math.pi * k / K
        z = torch.tensor([-math.cos(th), 0.0, -math.sin(th)])
        x = torch.tensor([-z[2], 0.0, z[0]])
        Rm = torch.stack([x, torch.tensor([0.0, 1.0, 0.0]), z])
        pos = -4.0 * z
        rows.append(torch.cat([torch.cat([Rm, (-Rm @ pos).unsqueeze(1)], 1).reshape(-1),
                               torch.tensor([1100.0, 1100.0, 960.0, 540.0, 1920.0, 1080.0])]))
    cams = torch.stack(rows).to(dev)
    flt = pkg.Filter3D(n, dev)
    ra = N.GsFilter3dRateArgs(n, xyz.data_ptr(), 3, cams.data_ptr(), K, 0.2, 0.15, flt.max_rate.data_ptr())
    stream = torch.cuda.current_stream().cuda_stream
    N.check(lib.gs_filter3d_accumulate(C.byref(ra), stream), "rate")
    flt.values = torch.where(flt.max_rate > 0, math.sqrt(0.2) / flt.max_rate, torch.zeros_like(flt.max_rate))
    f = flt.values
    s_out, o_out, d_s, d_o = torch.empty_like(s), torch.empty_like(o), torch.empty_like(s), torch.empty_like(o)
    ma = N.GsFilter3dArgs(n, s.data_ptr(), o.data_ptr(), f.data_ptr(), s_out.data_ptr(), o_out.data_ptr(),
                          g_s.data_ptr(), g_o.data_ptr(), d_s.data_ptr(), d_o.data_ptr())
    rate_t = torch.zeros(n, device=dev)
    variants = {
        "forward": lambda: N.check(lib.gs_filter3d_forward(C.byref(ma), stream), "forward"),
        "backward": lambda: N.check(lib.gs_filter3d_backward(C.byref(ma), stream), "backward"),
        "rate": lambda: N.check(lib.gs_filter3d_accumulate(C.byref(ra), stream), "rate"),
        "forward_torch": lambda: torch_forward(s, o, f),
        "backward_torch": lambda: torch_backward(s, o, f, g_s, g_o),
        "rate_torch": lambda: torch_rate(xyz, cams, 0.2, 0.15, rate_t),
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
            reps = a.reps if not name.endswith("rate_torch") else max(1, a.reps // 20)
            t = timed(call, reps)
            if r:
                times[name].append(t)
    # the torch maps say what the kernels say (fp32 against fp32)
    ts, to = torch_forward(s, o, f)
    lib.gs_filter3d_forward(C.byref(ma), stream)
    torch.cuda.synchronize()
    agree = {"s_out": float((ts - s_out).abs().max()), "o_out": float((to - o_out).abs().max()),
             "rate_rel": float(((rate_t - flt.max_rate).abs() / flt.max_rate.clamp_min(1e-30)).max())}
    bytes_ = {"forward": 36 * n, "backward": 52 * n, "rate": 16 * n + 72 * K}
    res = {"gaussians": n, "cameras": K, "reps": a.reps, "rounds": a.rounds,
           "us": {k: round(statistics.median(v), 2) for k, v in times.items()},
           "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
           "bytes": bytes_,
           "hbm_us_at_8.0TBs": {k: round(b / HBM_SPEC * 1e6, 2) for k, b in bytes_.items()},
           "hbm_us_at_6.29TBs": {k: round(b / HBM_COPY * 1e6, 2) for k, b in bytes_.items()},
           "seen": int((flt.max_rate > 0).sum()), "torch_minus_kernel": agree}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
