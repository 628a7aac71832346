"""The cost of TSDF fusion and mesh extraction at an N^3 colour volume (default
256^3) and V views of W x H (default 8 of 1920 x 1080): gs_tsdf_integrate (the
V views in one launch, and as V launches of one view), gs_mesh_classify and
gs_mesh_emit through the C ABI, and in the same run the same maps composed
from torch ops -- the fusion as points x view, gather and where per view; the
classification as shifted slices of the side and validity masks; the vertices
as nonzero, a gather of the corners and the crossings' mean (the faces have
no torch counterpart here).  The scene is a unit sphere seen from a ring of
cameras 4 units away: analytic depth maps, alpha 1 on the sphere, the normal as
colour.  Each variant is timed with device events around `--reps` back-to-back
calls, the variants alternating over `--rounds` rounds after a warm-up of
every variant; the figure is the median round's time per call, the spread the
rounds' min..max.  Beside each kernel: the time its bytes need at the HBM peak
(8.0 TB/s spec, 6.29 TB/s measured for a float4 copy).  Under
`rocprofv3 --kernel-trace --stats` the kernels' own times are those of
k_tsdf_integrate, k_mesh_classify, k_mesh_vertices and k_mesh_faces; `--only`
restricts a run to one of them.

    python tools/tsdf_bench.py [--n 256] [--views 8] [--width 1920] [--height 1080] [--reps 20] [--rounds 5]
                               [--only integrate|classify|emit] [--no-torch]

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


class RingCamera:
    def __init__(self, W, H, fovy, eye):
        self._width, self._height = W, H
        self._FoVy = fovy
        self._FoVx = 2 * math.atan(math.tan(fovy / 2) * W / H)
        eye = torch.tensor(eye, dtype=torch.float64)
        fwd = -eye / eye.norm()
        right = torch.linalg.cross(fwd, torch.tensor([0.0, 0.0, 1.0], dtype=torch.float64))
        right = right / right.norm()
        R = torch.stack([right, torch.linalg.cross(right, fwd), fwd])
        wv = torch.eye(4, dtype=torch.float64)
        wv[:3, :3], wv[:3, 3] = R, -R @ eye
        self.world_view_transform = wv.float()
        self.eye, self.R = eye.float(), R.float()


def sphere_maps(cam, dev):
    """(depth, alpha, image) of the unit sphere: the z depth of the ray's first hit."""
    W, H = cam._width, cam._height
    f = 0.5 * H / math.tan(cam._FoVy / 2)
    v, u = torch.meshgrid(torch.arange(H, device=dev, dtype=torch.float32),
                          torch.arange(W, device=dev, dtype=torch.float32), indexing="ij")
    d_cam = torch.stack([(u - W / 2) / f, -(v - H / 2) / f, torch.ones_like(u)], -1)
    w = d_cam @ cam.R.to(dev)  # R^T d
    eye = cam.eye.to(dev)
    a, b, c = (w * w).sum(-1), 2 * (w @ eye), float(eye @ eye) - 1.0
    disc = b * b - 4 * a * c
    hit = disc > 0
    t = torch.where(hit, (-b - disc.clamp_min(0).sqrt()) / (2 * a), torch.zeros_like(a))
    normal = eye + t[..., None] * w
    image = torch.where(hit[None], 0.5 + 0.5 * normal.permute(2, 0, 1), torch.zeros(3, H, W, device=dev))
    return t.contiguous(), hit.float().contiguous(), image.contiguous()


def torch_integrate(vol, P, rows, depth, alpha, image, alpha_min, depth_max):
    """The fusion composed from torch ops, view by view, over every node at once."""
    V, H, W = depth.shape
    t, w, col = vol.tsdf.reshape(-1), vol.weight.reshape(-1), vol.color.reshape(3, -1)
    for v in range(V):
        r = rows[v]
        cam = P @ r[:12].reshape(3, 4)[:, :3].T + r[:12].reshape(3, 4)[:, 3]
        Z = cam[:, 2]
        px, py = r[12] * cam[:, 0] / Z + r[14], -r[13] * cam[:, 1] / Z + r[15]
        u, vv = torch.floor(px + 0.5), torch.floor(py + 0.5)
        ok = (Z > vol.near) & (u >= 0) & (u < W) & (vv >= 0) & (vv < H)
        at = (vv.clamp(0, H - 1) * W + u.clamp(0, W - 1)).long()
        d = depth[v].reshape(-1)[at]
        s = d - Z
        ok &= (d > 0) & (d <= depth_max) & (alpha[v].reshape(-1)[at] >= alpha_min) & (s >= -vol.trunc)
        tau = (s / vol.trunc).clamp_max(1.0)
        w1 = w + 1
        t = torch.where(ok, (t * w + tau) / w1, t)
        col = torch.where(ok[None], (col * w + image[v].reshape(3, -1)[:, at]) / w1, col)
        w = torch.where(ok, w1, w)
    return t, w, col


def torch_classify(tsdf, weight, min_weight):
    """Active cells and the nodes' edge masks from shifted slices."""
    inside, ok = tsdf < 0, weight >= min_weight
    c = lambda a, dz, dy, dx: a[dz:a.shape[0] - 1 + dz, dy:a.shape[1] - 1 + dy, dx:a.shape[2] - 1 + dx]
    offs = [(dz, dy, dx) for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)]
    valid = torch.stack([c(ok, *o) for o in offs]).all(0)
    n_in = torch.stack([c(inside, *o) for o in offs]).sum(0)
    active = valid & (n_in > 0) & (n_in < 8)
    vp = torch.nn.functional.pad(valid, (1, 1, 1, 1, 1, 1))  # vp[k + 1, j + 1, i + 1] = valid[k, j, i]
    nz, ny, nx = tsdf.shape
    cell = lambda dz, dy, dx: vp[1 + dz:1 + dz + nz, 1 + dy:1 + dy + ny, 1 + dx:1 + dx + nx]
    diff = lambda dim: torch.nn.functional.pad(inside.narrow(dim, 0, inside.shape[dim] - 1) !=
                                               inside.narrow(dim, 1, inside.shape[dim] - 1),
                                               [0, 0] * (2 - dim) + [0, 1])
    mx = diff(2) & cell(-1, -1, 0) & cell(-1, 0, 0) & cell(0, 0, 0) & cell(0, -1, 0)
    my = diff(1) & cell(-1, 0, -1) & cell(0, 0, -1) & cell(0, 0, 0) & cell(-1, 0, 0)
    mz = diff(0) & cell(0, -1, -1) & cell(0, -1, 0) & cell(0, 0, 0) & cell(0, 0, -1)
    mask = mx.to(torch.uint8) | (my.to(torch.uint8) << 1) | (mz.to(torch.uint8) << 2)
    return active, mask


def torch_vertices(vol, active):
    """The vertices of the active cells: nonzero, a gather of the 8 corners, the crossings' mean."""
    k, j, i = torch.nonzero(active, as_tuple=True)
    f = {(dx, dy, dz): vol.tsdf[k + dz, j + dy, i + dx] for dz in (0, 1) for dy in (0, 1) for dx in (0, 1)}
    s, n = torch.zeros(len(k), 3, device=k.device), torch.zeros(len(k), device=k.device)
    for axis in range(3):
        for o0 in (0, 1):
            for o1 in (0, 1):
                a = [0, 0, 0]
                others = [d for d in range(3) if d != axis]
                a[others[0]], a[others[1]] = o0, o1
                b = list(a)
                b[axis] = 1
                fa, fb = f[tuple(a)], f[tuple(b)]
                cross = (fa < 0) != (fb < 0)
                q = torch.tensor(a, device=k.device, dtype=torch.float32).expand(len(k), 3).clone()
                q[:, axis] = fa / (fa - fb)
                s += torch.where(cross[:, None], q, torch.zeros_like(q))
                n += cross
    origin = torch.tensor(vol.origin, device=k.device)
    return origin + vol.voxel_size * (torch.stack([i, j, k], 1) + s / n[:, None])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--views", type=int, default=8)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--only", choices=["integrate", "classify", "emit"], default=None)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    import __graft_entry__ as ge
    pkg = ge.load_package()
    N = pkg._native
    lib = N.load()
    dev = torch.device("cuda", 0)
    n, V, W, H = a.n, a.views, a.width, a.height
    h = 2.6 / (n - 1)
    vol = pkg.TSDFVolume((-1.3,) * 3, h, (n, n, n), dev)
    cams = [RingCamera(W, H, 0.7, (4 * math.cos(2 * math.pi * i / V) * math.cos(0.4), 4 * math.sin(2 * math.pi * i / V) * math.cos(0.4),
                                   4 * math.sin(0.4))) for i in range(V)]
    maps = [sphere_maps(c, dev) for c in cams]
    depth, alpha, image = (torch.stack([m[k] for m in maps]) for k in range(3))
    rows = torch.tensor([pkg.filter3d.camera_row(c)[:16] for c in cams], dtype=torch.float32).to(dev)
    stream = torch.cuda.current_stream().cuda_stream

    def args_for(v0, v1):
        return N.GsTsdfIntegrateArgs(vol._vol(), v1 - v0, W, H, rows[v0:].data_ptr(), depth[v0:].data_ptr(),
                                     alpha[v0:].data_ptr(), image[v0:].data_ptr(), vol.near, vol.trunc, 0.5, float("inf"))
    batched, single = args_for(0, V), [args_for(v, v + 1) for v in range(V)]

    def integrate_batched():
        N.check(lib.gs_tsdf_integrate(C.byref(batched), stream), "gs_tsdf_integrate")

    def integrate_single():
        for s in single:
            N.check(lib.gs_tsdf_integrate(C.byref(s), stream), "gs_tsdf_integrate")

    # the volume the extraction is timed on: the V views fused once into a fresh volume
    integrate_batched()
    updated = int((vol.weight > 0).sum())
    first = {k: v.clone() for k, v in vol.state().items()}
    vol.reset()
    integrate_single()
    same_bits = all(torch.equal(first[k].view(torch.int32), v.view(torch.int32)) for k, v in vol.state().items())
    nodes, cells = n ** 3, (n - 1) ** 3
    cell_active = torch.empty(cells, dtype=torch.uint8, device=dev)
    node_tris, node_mask = torch.empty(nodes, dtype=torch.uint8, device=dev), torch.empty(nodes, dtype=torch.uint8, device=dev)
    frozen = pkg.TSDFVolume((-1.3,) * 3, h, (n, n, n), dev)  # (the timed fusion keeps adding views to `vol`)
    frozen.load_state(first)
    ma = N.GsMeshArgs(frozen._vol(), 1.0, cell_active.data_ptr(), node_tris.data_ptr(), node_mask.data_ptr())
    N.check(lib.gs_mesh_classify(C.byref(ma), stream), "gs_mesh_classify")
    cell_rank, node_faces = torch.cumsum(cell_active, 0, dtype=torch.int32), torch.cumsum(node_tris, 0, dtype=torch.int32)
    vn, fn = int(cell_rank[-1]), int(node_faces[-1])
    vertices, colors = torch.empty(vn, 3, device=dev), torch.empty(vn, 3, device=dev)
    faces = torch.empty(fn, 3, dtype=torch.int32, device=dev)
    ma.cell_rank, ma.node_faces, ma.num_vertices, ma.num_faces = cell_rank.data_ptr(), node_faces.data_ptr(), vn, fn
    ma.vertices, ma.colors, ma.faces = vertices.data_ptr(), colors.data_ptr(), faces.data_ptr()
    P = None

    def integrate_torch():
        nonlocal P
        if P is None:
            k, j, i = torch.meshgrid(*(torch.arange(n, device=dev, dtype=torch.float32),) * 3, indexing="ij")
            P = (torch.tensor(vol.origin, device=dev) + h * torch.stack([i, j, k], -1)).reshape(-1, 3)
        with torch.no_grad():
            return torch_integrate(frozen, P, rows, depth, alpha, image, 0.5, float("inf"))

    def classify_torch():
        return torch_classify(frozen.tsdf, frozen.weight, 1.0)
    active_t = None

    def emit_torch():
        return torch_vertices(frozen, active_t)
    variants = {
        "integrate": {"tsdf_integrate_batched": integrate_batched, "tsdf_integrate_single_views": integrate_single,
                      "tsdf_integrate_torch": integrate_torch},
        "classify": {"mesh_classify": lambda: N.check(lib.gs_mesh_classify(C.byref(ma), stream), "gs_mesh_classify"),
                     "mesh_classify_torch": classify_torch},
        "emit": {"mesh_emit": lambda: N.check(lib.gs_mesh_emit(C.byref(ma), stream), "gs_mesh_emit"),
                 "mesh_emit_vertices_torch": emit_torch},
    }
    chosen = {k: f for group, fs in variants.items() if a.only in (None, group) for k, f in fs.items()
              if not (a.no_torch and k.endswith("torch"))}
    agree = {}
    if "mesh_emit_vertices_torch" in chosen or "mesh_classify_torch" in chosen:
        active_t, mask_t = classify_torch()
        agree["classify_same_as_torch"] = bool(torch.equal(active_t.reshape(-1).to(torch.uint8), cell_active) and
                                               torch.equal(mask_t.reshape(-1), node_mask))
    if "mesh_emit_vertices_torch" in chosen:
        N.check(lib.gs_mesh_emit(C.byref(ma), stream), "gs_mesh_emit")
        agree["vertices_minus_torch"] = float((emit_torch() - vertices).abs().max())
    if "tsdf_integrate_torch" in chosen:
        t_t, w_t, _ = integrate_torch()  # (from `frozen`: V more views on top of the first V)
        again = pkg.TSDFVolume((-1.3,) * 3, h, (n, n, n), dev)
        again.load_state(first)
        ag = N.GsTsdfIntegrateArgs(again._vol(), V, W, H, rows.data_ptr(), depth.data_ptr(), alpha.data_ptr(),
                                   image.data_ptr(), vol.near, vol.trunc, 0.5, float("inf"))
        N.check(lib.gs_tsdf_integrate(C.byref(ag), stream), "gs_tsdf_integrate")
        same_w = w_t == again.weight.reshape(-1)
        agree["integrate_weights_differing_from_torch"] = int((~same_w).sum())
        agree["integrate_tsdf_minus_torch"] = float((t_t - again.tsdf.reshape(-1))[same_w].abs().max())
        del again, t_t, w_t

    def timed(call, reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(reps):
            call()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) * 1e3 / reps

    times = {k: [] for k in chosen}
    for r in range(a.rounds + 1):  # round 0: the warm-up of every variant
        for name, call in chosen.items():
            tm = timed(call, a.reps if not name.endswith("torch") else max(1, a.reps // 10))
            if r:
                times[name].append(tm)
    px = W * H
    bytes_ = {"tsdf_integrate_batched": 40 * updated + 20 * px * V,          # 20 B read + 20 B written per updated node
              "mesh_classify": 8 * nodes + 2 * nodes + cells,
              # a flag per cell and a mask per node; per vertex its rank, 8 corners of tsdf and colour, 24 B out;
              # per emitting edge the node's offset and side, four ranks, two triangles
              "mesh_emit": cells + nodes + (4 + 128 + 24) * vn + (8 + 16 + 24) * (fn // 2)}
    # (one-view launches read and write a node once per view that updates it: the sum of the first fusion's weights)
    bytes_["tsdf_integrate_single_views"] = 40 * int(first["weight"].sum()) + 20 * px * V
    bytes_ = {k: v for k, v in bytes_.items() if k in chosen}
    res = {"n": n, "views": V, "width": W, "height": H, "reps": a.reps, "rounds": a.rounds,
           "updated_nodes": updated, "vertices": vn, "faces": fn, "batched_equals_single_views_bitwise": bool(same_bits),
           "us": {k: round(statistics.median(v), 2) for k, v in times.items()},
           "us_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in times.items()},
           "bytes": bytes_,
           "hbm_us_at_8.0TBs": {k: round(b / HBM_SPEC * 1e6, 2) for k, b in bytes_.items()},
           "hbm_us_at_6.29TBs": {k: round(b / HBM_COPY * 1e6, 2) for k, b in bytes_.items()},
           "torch_agreement": agree}
    print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
