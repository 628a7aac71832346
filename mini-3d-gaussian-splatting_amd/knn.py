"""Exact k-nearest neighbours of a point cloud, and 3DGS's start-up scale.

`mean_knn_dist2(points, 3)` is simple_knn's distCUDA2: the mean squared
distance of every point to its three nearest neighbours, whose root is the
initial scale of a Gaussian in 3DGS, gsplat, 2DGS, Mip-Splatting and 3DGS-MCMC
(GaussianModel.create_from_points(..., scale_init="knn")).

The result is defined apart from how it is found (include/gsplat_mi355x.h,
"k-nearest neighbours"): with d2(a, b) = ((dx dx) + (dy dy)) + (dz dz) of the
fp32 differences, row i holds the k smallest pairs (d2(p_i, p_j), j), j != i,
in lexicographic order -- equal distances resolve to the smaller row, a
duplicate of p_i elsewhere is a neighbour at distance 0 -- padded with
+inf / -1 where the cloud has fewer than k other points.

HIP tensors go through gs_knn on the current stream (Morton-ordered boxes of
256 points, AABB culls that never drop a pair they should keep: about
N x a few thousand distance evaluations).  CPU tensors go through a chunked
torch brute force with the same definition, down to the tie rule: O(N^2), for
the small clouds of tests and CPU-side tooling, not for a million points.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Tuple

import torch

from . import _native as N

_CPU_CHUNK_ELEMS = 1 << 22  # distances held at once by the CPU path


def _check(points, k) -> Tuple[torch.Tensor, int]:
    if not isinstance(points, torch.Tensor):
        raise ValueError(f"points must be a torch tensor of shape [N, 3], got {type(points).__name__}")
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"points must have shape [N, 3], got {tuple(points.shape)}")
    if not points.is_floating_point():
        raise ValueError(f"points must be floating point, got {points.dtype}")
    if isinstance(k, bool) or not isinstance(k, int) or not 1 <= k <= N.GS_KNN_MAX_K:
        raise ValueError(f"k must be an integer in 1..{N.GS_KNN_MAX_K}, got {k!r}")
    if points.device.type not in ("cpu", "cuda"):
        raise ValueError(f"points must be on the CPU or a HIP device, got {points.device}")
    points = points.detach().to(torch.float32).contiguous()
    if points.shape[0] and not bool(torch.isfinite(points).all()):  # (the call's one host read)
        raise ValueError("points must be finite")
    return points, k


def _knn_cpu(p: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """The definition, by brute force: a stable sort of each row of distances
    orders equal ones by row index."""
    n = p.shape[0]
    dist2 = torch.full((n, k), float("inf"), dtype=torch.float32)
    index = torch.full((n, k), -1, dtype=torch.int32)
    if n < 2:
        return dist2, index
    m = min(k + 1, n)  # the query itself may sit among the first k + 1
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    step = max(1, _CPU_CHUNK_ELEMS // n)
    for r0 in range(0, n, step):
        r1 = min(n, r0 + step)
        dx, dy, dz = x[r0:r1, None] - x[None, :], y[r0:r1, None] - y[None, :], z[r0:r1, None] - z[None, :]
        d = (dx * dx + dy * dy) + dz * dz
        ds, js = torch.sort(d, dim=1, stable=True)
        ds, js = ds[:, :m], js[:, :m]
        drop = js == torch.arange(r0, r1)[:, None]
        drop[~drop.any(1), m - 1] = True  # (the query is further down: the first m - 1 stand)
        keep = ~drop
        dist2[r0:r1, :m - 1] = ds[keep].view(r1 - r0, m - 1)
        index[r0:r1, :m - 1] = js[keep].view(r1 - r0, m - 1).to(torch.int32)
    return dist2, index


def _mean_of(dist2: torch.Tensor, n: int, k: int) -> torch.Tensor:
    """gs_knn's mean_dist2 from a [N, k] result: ascending fp32 sum / count."""
    found = min(k, n - 1)
    if found <= 0:
        return torch.zeros(n, dtype=torch.float32, device=dist2.device)
    s = dist2[:, 0].clone()
    for c in range(1, found):
        s += dist2[:, c]
    return s / float(found)


def _knn_hip(p: torch.Tensor, k: int, want_dist: bool, want_index: bool, want_mean: bool):
    n, dev = p.shape[0], p.device
    lib = N.load()
    with torch.cuda.device(dev):
        ws = torch.empty((max(int(lib.gs_knn_workspace_bytes(n)), 16),), dtype=torch.uint8, device=dev)
        dist2 = torch.empty((n, k), dtype=torch.float32, device=dev) if want_dist else None
        index = torch.empty((n, k), dtype=torch.int32, device=dev) if want_index else None
        mean = torch.empty((n,), dtype=torch.float32, device=dev) if want_mean else None
        a = N.GsKnnArgs(n, k, N.ptr(p), N.ptr(dist2), N.ptr(index), N.ptr(mean), N.ptr(ws), ws.numel())
        N.check(lib.gs_knn(C.byref(a), N.stream_ptr(dev)), "gs_knn")
    return dist2, index, mean


@torch.no_grad()
def knn(points: torch.Tensor, k: int = 3, return_index: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
    """(dist2 [N, k] float32 ascending, index [N, k] int32) of every point's k
    nearest other points (the module's docstring has the exact definition);
    index is None with return_index=False.  ValueError for a shape other than
    [N, 3], k outside 1..16 or non-finite coordinates."""
    p, k = _check(points, k)
    n = p.shape[0]
    if n == 0:
        return (torch.empty((0, k), dtype=torch.float32, device=p.device),
                torch.empty((0, k), dtype=torch.int32, device=p.device) if return_index else None)
    if p.is_cuda:
        dist2, index, _ = _knn_hip(p, k, True, bool(return_index), False)
        return dist2, index
    dist2, index = _knn_cpu(p, k)
    return dist2, (index if return_index else None)


@torch.no_grad()
def mean_knn_dist2(points: torch.Tensor, k: int = 3) -> torch.Tensor:
    """[N] float32: the mean of d2 to the min(k, N - 1) nearest other points
    (0 for a single point), summed ascending in fp32 -- distCUDA2 at k = 3."""
    p, k = _check(points, k)
    n = p.shape[0]
    if n == 0:
        return torch.empty((0,), dtype=torch.float32, device=p.device)
    if p.is_cuda:
        return _knn_hip(p, k, False, False, True)[2]
    return _mean_of(_knn_cpu(p, k)[0], n, k)
