"""The statements the MCMC density-control kernels are checked against
(include/gsplat_mi355x.h, "MCMC density control"), in float64 and Python
integers: the relocation with math.comb, the sampling as an integer product
and a sorted search, the position noise from the densify test's normals, and
the regularisers by torch autograd.  Not in the reference."""
import math

import numpy as np
import torch

from test_densify import mix64, normals_of

MAX_OPACITY = 1.0 - 2.0 ** -24
MAX_RATIO = 51


def sample_statement(cdf, num_samples, seed):
    """idx [num_samples] and counts [n]: r = (mix64(seed ^ mix64(j)) * total) >> 64
    in Python integers, then the smallest i with cdf[i] > r."""
    cdf = np.asarray(cdf, dtype=np.int64)
    total = int(cdf[-1])
    r = np.array([(mix64(seed ^ mix64(j)) * total) >> 64 for j in range(num_samples)], dtype=np.int64)
    idx = np.searchsorted(cdf, r, side="right").astype(np.int32)
    return idx, np.bincount(idx, minlength=cdf.size).astype(np.int32)


def relocation_denominator(x, ratio):
    """D = sum_{i=1..R} sum_{k=0..i-1} C(i-1, k) (-1)^k x^(k+1) / sqrt(k+1)."""
    d = 0.0
    for i in range(1, ratio + 1):
        for k in range(i):
            d += math.comb(i - 1, k) * (-1.0) ** k * x ** (k + 1) / math.sqrt(k + 1)
    return d


def relocate_values(opacity_logit, log_scale, count, min_opacity):
    """One sampled row: (new opacity logit, new log-scales [3]) in float64."""
    ratio = min(int(count) + 1, MAX_RATIO)
    o = min(1.0 / (1.0 + math.exp(-float(opacity_logit))), MAX_OPACITY)
    x = 1.0 - (1.0 - o) ** (1.0 / ratio)
    d = relocation_denominator(x, ratio)
    xc = min(max(x, min_opacity), MAX_OPACITY)
    return math.log(xc / (1.0 - xc)), np.asarray(log_scale, dtype=np.float64) + math.log(o / d)


def relocate_statement(opacity_logit, log_scale, idx, counts, min_opacity):
    """Per sample j: the values rows idx[j] and dst[j] get, [S] and [S, 3] float64."""
    op = np.empty(len(idx))
    sc = np.empty((len(idx), 3))
    cache = {}
    for j, s in enumerate(np.asarray(idx).tolist()):
        if s not in cache:
            cache[s] = relocate_values(opacity_logit[s], log_scale[s], counts[s], min_opacity)
        op[j], sc[j] = cache[s]
    return op, sc


def noise_statement(xyz, log_scale, rotation, opacity_logit, scale, seed, steepness=100.0, midpoint=0.005):
    """The position change Sigma eps * (gate * scale), [n, 3] float64, from fp32 inputs."""
    xyz, s, q, op = (np.asarray(t, dtype=np.float64) for t in (xyz, log_scale, rotation, opacity_logit))
    n = xyz.shape[0]
    q = q / np.maximum(np.linalg.norm(q, axis=1, keepdims=True), 1e-12)
    w, x, y, z = q.T
    R = np.stack([1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y),
                  2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x),
                  2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)], -1).reshape(n, 3, 3)
    sigma = R @ (np.exp(s)[:, :, None] ** 2 * np.transpose(R, (0, 2, 1)))
    o = 1.0 / (1.0 + np.exp(-op.reshape(n)))
    gate = 1.0 / (1.0 + np.exp(-steepness * (midpoint - o)))
    eps = normals_of(seed, n)
    return np.einsum("nij,nj->ni", sigma, eps) * (gate * scale)[:, None]


def regularizer_grads(opacity_logit, log_scale, lambda_opacity, lambda_scale):
    """d/d(opacity), d/d(scaling) of lambda_o mean(sigmoid(opacity)) + lambda_s mean(exp(scaling)), float64."""
    op = opacity_logit.detach().double().cpu().requires_grad_(True)
    sc = log_scale.detach().double().cpu().requires_grad_(True)
    (lambda_opacity * torch.sigmoid(op).mean() + lambda_scale * torch.exp(sc).mean()).backward()
    return op.grad, sc.grad
