"""The 3DGS-MCMC density control's launches over plain tensors (Kheradmand et
al. 2024; include/gsplat_mi355x.h, "MCMC density control"): weighted sampling,
relocation, position noise and the regularisers' gradients.  The model and the
optimizer build on these (GaussianModel.relocate_and_grow,
GaussianOptimizer.mcmc_*); nothing here allocates a parameter or reads a value
back to the host."""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence, Tuple

import torch

from . import _native as N

WEIGHT_SCALE = float(1 << 24)  # opacity -> integer weight: exact in fp32, so every rank and the CPU agree


def _dev(t: torch.Tensor, dtype, what: str) -> torch.Tensor:
    if not (t.is_cuda and t.dtype == dtype and t.is_contiguous()):
        raise RuntimeError(f"{what} must be a contiguous {dtype} tensor on a HIP device")
    return t


def opacity_cdf(opacity_logit: torch.Tensor, min_opacity: float) -> torch.Tensor:
    """The sampling weights' inclusive prefix sums: w = floor(sigmoid(opacity) * 2^24)
    where sigmoid(opacity) > min_opacity, else 0, as int64 (an integer sum: the
    same in any order)."""
    o = torch.sigmoid(opacity_logit.detach().reshape(-1))
    w = torch.where(o > min_opacity, torch.floor(o * WEIGHT_SCALE), torch.zeros_like(o)).to(torch.int64)
    return torch.cumsum(w, 0)


def mcmc_sample(cdf: torch.Tensor, num_samples: int, seed: int, idx: Optional[torch.Tensor] = None,
                counts: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
    """gs_mcmc_sample: `num_samples` rows drawn with replacement with probability
    proportional to the weights whose prefix sums `cdf` holds.  Returns (idx
    int32 [num_samples], counts int32 [n]); given tensors are written in place
    (counts is added to: the caller zeroes it)."""
    _dev(cdf, torch.int64, "cdf")
    n = cdf.numel()
    if idx is None:
        idx = torch.empty(num_samples, dtype=torch.int32, device=cdf.device)
    if counts is None:
        counts = torch.zeros(n, dtype=torch.int32, device=cdf.device)
    _dev(idx, torch.int32, "idx")
    _dev(counts, torch.int32, "counts")
    if idx.numel() != num_samples or counts.numel() != n:
        raise ValueError("idx must hold num_samples entries and counts one per cdf row")
    a = N.GsMcmcSampleArgs(n, int(num_samples), N.ptr(cdf), int(seed) & 0xFFFFFFFFFFFFFFFF, N.ptr(idx), N.ptr(counts))
    N.check(N.load().gs_mcmc_sample(C.byref(a), N.stream_ptr(cdf.device)), "gs_mcmc_sample")
    return idx, counts


def _arrays(ts: Sequence[Optional[torch.Tensor]]) -> N.GsModelArrays:
    return N.GsModelArrays(*[N.ptr(t) if t is not None and t.numel() else None for t in ts])


def mcmc_relocate(params: Sequence[torch.Tensor], idx: torch.Tensor, counts: torch.Tensor, dst: torch.Tensor,
                  min_opacity: float, adam_m: Optional[Sequence[Optional[torch.Tensor]]] = None,
                  adam_v: Optional[Sequence[Optional[torch.Tensor]]] = None) -> None:
    """gs_mcmc_relocate over the six parameter tensors (gs_model_arrays order),
    in place: row dst[j] becomes a copy of row idx[j] with the relocation's
    opacity and scale, which row idx[j] takes too; the given Adam moments of
    both rows become zero.  counts has one entry per row that can be sampled
    (rows past it only receive).  The caller guarantees distinct dst rows, none
    of them sampled."""
    rows = int(params[0].shape[0])
    for group in (params, adam_m or (), adam_v or ()):
        for t in group:
            if t is not None:
                _dev(t, torch.float32, "a parameter or moment")
                if t.shape[0] != rows:
                    raise ValueError("parameters and moments must have the same number of rows")
    for t, what in ((idx, "idx"), (counts, "counts"), (dst, "dst")):
        _dev(t, torch.int32, what)
    s = idx.numel()
    if dst.numel() != s or counts.numel() > rows:
        raise ValueError("dst must hold one row per sample, counts at most one entry per row")
    lib = N.load()
    ws = torch.empty((max(s, 1), 4), dtype=torch.float32, device=idx.device)
    a = N.GsMcmcRelocateArgs()
    a.n, a.rows, a.num_samples = counts.numel(), rows, s
    a.rest_floats = int(params[2][0].numel()) if rows else 0
    a.params = _arrays(params)
    a.adam_m = _arrays(adam_m if adam_m is not None else [None] * 6)
    a.adam_v = _arrays(adam_v if adam_v is not None else [None] * 6)
    a.idx, a.counts, a.dst, a.min_opacity = N.ptr(idx), N.ptr(counts), N.ptr(dst), float(min_opacity)
    a.workspace, a.workspace_bytes = N.ptr(ws), ws.numel() * 4
    N.check(lib.gs_mcmc_relocate(C.byref(a), N.stream_ptr(idx.device)), "gs_mcmc_relocate")


def mcmc_noise(xyz: torch.Tensor, scaling: torch.Tensor, rotation: torch.Tensor, opacity: torch.Tensor,
               scale: float, seed: int, gate_steepness: float = N.GS_MCMC_GATE_STEEPNESS,
               gate_midpoint: float = N.GS_MCMC_GATE_MIDPOINT) -> None:
    """gs_mcmc_noise: xyz += Sigma eps * (gate(opacity) * scale), in place, eps
    the counter-based normals of (seed, row, axis)."""
    for t in (xyz, scaling, rotation, opacity):
        _dev(t, torch.float32, "xyz, scaling, rotation and opacity")
    n = int(xyz.shape[0])
    if scaling.shape[0] != n or rotation.shape[0] != n or opacity.numel() != n:
        raise ValueError("xyz, scaling, rotation and opacity must have the same number of rows")
    a = N.GsMcmcNoiseArgs(n, N.ptr(xyz), N.ptr(scaling), N.ptr(rotation), N.ptr(opacity),
                          int(seed) & 0xFFFFFFFFFFFFFFFF, float(scale), float(gate_steepness), float(gate_midpoint))
    N.check(N.load().gs_mcmc_noise(C.byref(a), N.stream_ptr(xyz.device)), "gs_mcmc_noise")


def mcmc_regularize(opacity: torch.Tensor, scaling: torch.Tensor, d_opacity: Optional[torch.Tensor],
                    d_scaling: Optional[torch.Tensor], lambda_opacity: float, lambda_scale: float) -> None:
    """gs_mcmc_regularize: the gradients of lambda_opacity * mean(sigmoid(opacity))
    + lambda_scale * mean(exp(scaling)) added to d_opacity / d_scaling (None:
    that term is skipped)."""
    n = int(opacity.numel())
    for t in (opacity, scaling, d_opacity, d_scaling):
        if t is not None:
            _dev(t, torch.float32, "opacity, scaling and their gradients")
    if scaling.numel() != 3 * n or (d_opacity is not None and d_opacity.numel() != n) or \
            (d_scaling is not None and d_scaling.numel() != 3 * n):
        raise ValueError("opacity [n], scaling [n,3] and gradients of the same shapes")
    if not (math.isfinite(lambda_opacity) and math.isfinite(lambda_scale)):
        raise ValueError("the regularisers' weights must be finite")
    a = N.GsMcmcRegularizeArgs(n, N.ptr(opacity), N.ptr(scaling), N.ptr(d_opacity), N.ptr(d_scaling),
                               float(lambda_opacity), float(lambda_scale))
    N.check(N.load().gs_mcmc_regularize(C.byref(a), N.stream_ptr(opacity.device)), "gs_mcmc_regularize")


__all__ = ["opacity_cdf", "mcmc_sample", "mcmc_relocate", "mcmc_noise", "mcmc_regularize", "WEIGHT_SCALE"]
