"""Cost of the visibility-gated Adam step next to the dense one.

The six model tensors at n Gaussians with SH degree 3 (xyz 3, features_dc 3,
features_rest 45, scaling 3, rotation 4, opacity 1: 59 floats a Gaussian),
one launch each of
  * gs_adam_step (k_adam), the dense step;
  * gs_adam_step_rows (k_adam_rows) with every row visible, 30 % of the rows
    at random, 30 % in contiguous runs of 4096 rows, and no row.
The GPU is spun up first; then WARMUP + reps launches per variant, in that
order, timed with device events (median of the reps).  One JSON line: us per
launch, the bytes the update needs (28 B per updated element: p, g, m, v read,
p, m, v written; plus the mask bytes the row kernel reads, once per tensor) and
that over the time.

The same run under the profiler gives the kernel times:
    rocprofv3 --kernel-trace --stats -d <dir> -o run --output-format csv -- \\
        python tools/visible_adam_bench.py
    python tools/visible_adam_bench.py --trace <dir>/.../run_kernel_trace.csv
--trace reads the launches back in issue order: WARMUP + reps per variant.

usage: python tools/visible_adam_bench.py [--n 1000000] [--reps 20]"""
import argparse
import csv
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COLS = (3, 3, 45, 3, 4, 1)
WARMUP = 3
VARIANTS = ("dense", "rows_all", "rows_random30", "rows_runs30", "rows_none")
RUN = 4096


def masks(n, torch, dev):
    gen = torch.Generator().manual_seed(0)
    runs = (n + RUN - 1) // RUN
    on_runs = torch.rand(runs, generator=gen) < 0.3
    return {"rows_all": torch.ones(n, dtype=torch.uint8, device=dev),
            "rows_random30": (torch.rand(n, generator=gen) < 0.3).to(torch.uint8).to(dev),
            "rows_runs30": on_runs.repeat_interleave(RUN)[:n].to(torch.uint8).to(dev),
            "rows_none": torch.zeros(n, dtype=torch.uint8, device=dev)}


def run(n, reps):
    import torch
    import __graft_entry__ as ge
    pkg = ge.load_package()
    N = pkg._native
    lib = N.load()
    dev = torch.device("cuda", 0)
    gen = torch.Generator().manual_seed(1)
    t = [[torch.randn(n * c, generator=gen).to(dev) for _ in range(4)] for c in COLS]  # p, m, v, g
    for x in t:
        x[2].abs_()
    b1, b2 = 0.9, 0.999
    rows_args = N.GsAdamRowsArgs()
    dense_args = N.GsAdamArgs()
    for a in (rows_args.adam, dense_args):
        a.num_tensors, a.beta1, a.beta2, a.eps = len(COLS), b1, b2, 1e-15
        a.one_minus_beta1, a.one_minus_beta2 = 1.0 - b1, 1.0 - b2
        for k, (p, m, v, g) in enumerate(t):
            a.t[k] = N.GsAdamTensor(N.ptr(p), N.ptr(m), N.ptr(v), N.ptr(g), p.numel(), 1e-5, 1.0 - b1 ** 10,
                                    (1.0 - b2 ** 10) ** 0.5, None)
    rows_args.rows = n
    for k, c in enumerate(COLS):
        rows_args.cols[k] = c
    ms = masks(n, torch, dev)
    stream = N.stream_ptr()

    def launch(name):
        if name == "dense":
            N.check(lib.gs_adam_step(C.byref(dense_args), stream), "gs_adam_step")
        else:
            rows_args.row_mask = N.ptr(ms[name])
            N.check(lib.gs_adam_step_rows(C.byref(rows_args), stream), "gs_adam_step_rows")

    # spin-up: the clock ramps over the first tens of ms of load
    spin = torch.empty(64 << 20, device=dev)
    for _ in range(200):
        spin.add_(1.0)
    torch.cuda.synchronize()
    out = {"n": n, "floats_per_gaussian": sum(COLS), "reps": reps}
    for name in VARIANTS:
        for _ in range(WARMUP):
            launch(name)
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
        for a, b in ev:
            a.record()
            launch(name)
            b.record()
        torch.cuda.synchronize()
        us = statistics.median(a.elapsed_time(b) for a, b in ev) * 1e3
        visible = n if name == "dense" else int(ms[name].sum())
        need = sum(COLS) * 28 * visible + (0 if name == "dense" else len(COLS) * n)
        out[name] = {"us": round(us, 1), "visible_fraction": round(visible / n, 4), "needed_MB": round(need / 1e6, 1),
                     "needed_GBps": round(need / us / 1e3, 1)}
    print(json.dumps(out))
    return out


def trace(path, reps):
    rows = [r for r in csv.DictReader(open(path)) if "k_adam" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    per = WARMUP + reps
    assert len(rows) == per * len(VARIANTS), (len(rows), per)
    for i, name in enumerate(VARIANTS):
        chunk = rows[i * per + WARMUP:(i + 1) * per]
        kernel = "k_adam_rows" if "k_adam_rows" in chunk[0]["Kernel_Name"] else "k_adam"
        assert all((kernel == "k_adam_rows") == ("k_adam_rows" in r["Kernel_Name"]) for r in chunk)
        us = [(int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3 for r in chunk]
        print(f"{name:14s} {kernel:12s} calls {len(us):3d}  median {statistics.median(us):8.1f} us  "
              f"min {min(us):8.1f}  max {max(us):8.1f}")


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", default=None)
    args = ap.parse_args()
    if args.trace:
        trace(args.trace, args.reps)
    else:
        run(args.n, args.reps)
