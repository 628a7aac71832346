"""The projection stage alone: gs_project_forward / gs_project_backward called
through the C ABI on synthetic Gaussians and compared, per Gaussian, with the
fp64 statement of tests/project_reference.py (integer outputs exactly).

Tolerance (floats): per output tensor and case, each Gaussian's row-relative
error max_k |d - d64| / max_k |d64|; the kernel's median, p90, p99 and max must
each be <= 4 x the fp32 torch statement's same quantile on the same inputs,
+ 1e-7.  Rows whose fp64 value is all zero must be exactly zero.

Measured on an MI355X (kernel / fp32 statement, row-relative error against
fp64), full-size cases; forward tensors, d_xyz, d_scaling and d_rotation from
the training configuration (raw scale and rotation, DC colour), colour,
d_cov3d and d_sh_rest from the cov3d + SH degree 3 one:

population    tensor                   median                 p90                 p99                 max
plain         means2d      3.11e-08/3.11e-08   6.50e-08/6.50e-08   3.63e-07/3.63e-07   1.86e-06/1.86e-06
plain         conics       2.72e-07/2.72e-07   4.37e-06/4.41e-06   6.40e-05/6.30e-05   3.87e-04/3.48e-04
plain         radii        5.78e-08/5.85e-08   1.61e-07/1.67e-07   3.21e-07/3.22e-07   1.38e-06/8.27e-07
plain         Z            0.00e+00/0.00e+00   0.00e+00/0.00e+00   0.00e+00/0.00e+00   0.00e+00/0.00e+00
plain         d_xyz        2.54e-08/6.31e-08   4.67e-08/2.27e-06   1.08e-07/7.41e-05   2.37e-07/4.52e-04
plain         d_scaling    4.38e-08/5.84e-07   9.04e-08/1.14e-05   1.31e-07/1.42e-04   1.80e-07/6.44e-04
plain         d_rotation   6.55e-08/6.12e-07   1.51e-07/1.24e-05   3.22e-07/1.60e-04   6.86e-07/2.31e-03
plain         colour       5.08e-08/5.05e-08   9.39e-08/9.19e-08   1.68e-07/1.60e-07   2.88e-07/3.23e-07
plain         d_cov3d      3.24e-07/3.14e-07   6.32e-06/6.51e-06   7.64e-05/8.49e-05   4.04e-04/4.00e-04
plain         d_sh_rest    1.63e-07/1.49e-07   3.06e-07/2.80e-07   4.64e-07/4.78e-07   8.64e-07/1.02e-06
needles       means2d      3.11e-08/3.11e-08   6.60e-08/6.60e-08   4.28e-07/4.28e-07   1.87e-06/1.87e-06
needles       conics       6.85e-07/6.68e-07   1.61e-05/1.67e-05   1.54e-04/1.44e-04   5.54e-04/6.71e-04
needles       radii        6.04e-08/6.15e-08   1.72e-07/1.80e-07   3.68e-07/3.81e-07   1.11e-06/1.01e-06
needles       Z            0.00e+00/0.00e+00   0.00e+00/0.00e+00   0.00e+00/0.00e+00   0.00e+00/0.00e+00
needles       d_xyz        2.74e-08/1.33e-07   5.02e-08/1.10e-05   1.25e-07/2.06e-04   4.38e-07/9.69e-04
needles       d_scaling    4.29e-08/1.95e-06   8.81e-08/4.13e-05   1.26e-07/3.32e-04   1.49e-07/1.24e-03
needles       d_rotation   6.92e-08/1.92e-06   1.73e-07/4.27e-05   3.80e-07/4.22e-04   6.28e-07/4.48e-03
needles       colour       5.16e-08/5.02e-08   9.37e-08/8.92e-08   1.53e-07/1.48e-07   2.88e-07/2.88e-07
needles       d_cov3d      9.96e-07/9.98e-07   2.29e-05/2.64e-05   2.41e-04/2.43e-04   1.16e-03/1.26e-03
needles       d_sh_rest    1.60e-07/1.45e-07   3.04e-07/2.70e-07   4.57e-07/4.40e-07   9.45e-07/9.31e-07
quats         means2d      3.09e-08/3.09e-08   6.46e-08/6.46e-08   4.20e-07/4.20e-07   2.27e-06/2.27e-06
quats         conics       3.26e-07/3.18e-07   4.33e-06/4.48e-06   6.03e-05/5.59e-05   2.85e-04/2.62e-04
quats         radii        7.07e-08/7.10e-08   1.93e-07/1.94e-07   3.63e-07/3.54e-07   1.72e-06/2.04e-06
quats         Z            0.00e+00/0.00e+00   0.00e+00/0.00e+00   0.00e+00/0.00e+00   0.00e+00/0.00e+00
quats         d_xyz        2.64e-08/6.28e-08   4.83e-08/1.83e-06   1.07e-07/5.08e-05   1.93e-07/2.74e-04
quats         d_scaling    4.62e-08/5.90e-07   8.88e-08/1.19e-05   1.26e-07/1.56e-04   1.76e-07/5.24e-04
quats         d_rotation   6.37e-08/6.52e-07   1.49e-07/1.16e-05   3.58e-07/1.65e-04   5.52e-07/7.42e-04
quats         colour       5.35e-08/5.28e-08   9.38e-08/9.30e-08   1.66e-07/1.63e-07   3.38e-07/2.68e-07
quats         d_cov3d      3.38e-07/2.92e-07   6.74e-06/6.59e-06   1.14e-04/1.06e-04   3.48e-04/3.11e-04
quats         d_sh_rest    1.64e-07/1.51e-07   3.14e-07/2.83e-07   4.92e-07/4.49e-07   9.42e-07/8.67e-07
near_behind   means2d      3.00e-08/3.00e-08   6.71e-08/6.71e-08   2.67e-07/2.67e-07   6.36e-06/6.36e-06
near_behind   conics       1.85e-07/1.87e-07   7.50e-07/7.51e-07   3.28e-06/3.75e-06   1.99e-05/2.11e-05
near_behind   radii        4.78e-08/4.57e-08   1.62e-07/1.57e-07   3.12e-07/3.10e-07   6.43e-07/7.51e-07
near_behind   Z            0.00e+00/0.00e+00   0.00e+00/0.00e+00   0.00e+00/0.00e+00   0.00e+00/0.00e+00
near_behind   d_xyz        2.36e-08/4.95e-08   4.42e-08/2.00e-07   9.90e-08/2.76e-06   7.77e-07/3.34e-05
near_behind   d_scaling    4.46e-08/3.66e-07   9.21e-08/1.77e-06   1.31e-07/8.53e-06   2.03e-07/4.24e-05
near_behind   d_rotation   6.11e-08/4.11e-07   1.21e-07/2.15e-06   2.21e-07/1.42e-05   5.95e-07/8.20e-05
near_behind   colour       5.17e-08/5.04e-08   9.24e-08/9.03e-08   1.35e-07/1.26e-07   1.83e-07/2.03e-07
near_behind   d_cov3d      2.30e-07/2.13e-07   1.02e-06/1.09e-06   5.61e-06/7.19e-06   6.12e-05/3.94e-05
near_behind   d_sh_rest    1.60e-07/1.46e-07   3.09e-07/2.75e-07   5.00e-07/4.74e-07   9.20e-07/8.68e-07
posed         means2d      4.14e-08/4.14e-08   1.13e-07/1.13e-07   7.46e-07/7.46e-07   4.93e-06/4.93e-06
posed         conics       3.38e-07/3.36e-07   5.31e-06/5.64e-06   7.46e-05/6.77e-05   4.80e-04/4.41e-04
posed         radii        6.24e-08/6.42e-08   1.79e-07/1.81e-07   3.57e-07/3.44e-07   6.04e-06/6.35e-06
posed         Z            2.40e-08/2.40e-08   5.69e-08/5.69e-08   8.52e-08/8.52e-08   1.17e-07/1.17e-07
posed         d_xyz        2.62e-08/9.26e-08   4.73e-08/2.25e-06   8.93e-08/6.54e-05   5.74e-07/1.27e-03
posed         d_scaling    4.47e-08/6.95e-07   9.25e-08/1.45e-05   1.34e-07/1.37e-04   1.77e-07/8.82e-04
posed         d_rotation   6.55e-08/7.43e-07   1.60e-07/1.58e-05   3.51e-07/2.16e-04   6.69e-07/2.22e-03
posed         colour       5.16e-08/5.11e-08   9.34e-08/9.13e-08   1.58e-07/1.59e-07   2.87e-07/2.87e-07
posed         d_cov3d      4.72e-07/4.58e-07   8.88e-06/9.15e-06   1.13e-04/9.96e-05   5.50e-04/6.17e-04
posed         d_sh_rest    1.64e-07/1.52e-07   3.07e-07/2.82e-07   4.95e-07/4.83e-07   8.13e-07/7.68e-07
radius_clamp  means2d      3.06e-08/3.06e-08   6.59e-08/6.59e-08   3.13e-07/3.13e-07   3.70e-06/3.70e-06
radius_clamp  conics       1.37e-07/1.41e-07   8.64e-07/8.61e-07   2.99e-05/1.99e-05   2.86e-04/2.82e-04
radius_clamp  radii        0.00e+00/0.00e+00   1.07e-07/1.05e-07   2.56e-07/2.61e-07   7.02e-07/6.78e-07
radius_clamp  Z            0.00e+00/0.00e+00   0.00e+00/0.00e+00   0.00e+00/0.00e+00   0.00e+00/0.00e+00
radius_clamp  d_xyz        2.76e-08/7.31e-08   5.42e-08/7.02e-07   1.28e-07/2.39e-05   2.74e-07/7.15e-04
radius_clamp  d_scaling    4.12e-08/2.92e-07   8.67e-08/2.36e-06   1.30e-07/6.02e-05   1.79e-07/5.65e-04
radius_clamp  d_rotation   5.87e-08/3.51e-07   1.27e-07/2.68e-06   2.55e-07/6.12e-05   6.04e-07/8.00e-04
radius_clamp  colour       5.05e-08/4.94e-08   9.48e-08/9.28e-08   1.59e-07/1.53e-07   2.81e-07/2.81e-07
radius_clamp  d_cov3d      1.57e-07/1.63e-07   1.19e-06/1.21e-06   3.75e-05/3.65e-05   4.81e-04/4.73e-04
radius_clamp  d_sh_rest    1.55e-07/1.45e-07   3.09e-07/2.74e-07   4.96e-07/4.54e-07   7.64e-07/1.16e-06
saturated     means2d      2.93e-08/2.93e-08   6.34e-08/6.34e-08   4.52e-07/4.52e-07   1.44e-06/1.44e-06
saturated     conics       2.71e-07/2.82e-07   4.47e-06/5.01e-06   5.49e-05/5.85e-05   2.84e-04/2.72e-04
saturated     radii        5.61e-08/5.81e-08   1.64e-07/1.69e-07   3.19e-07/3.19e-07   3.23e-06/3.23e-06
saturated     Z            0.00e+00/0.00e+00   0.00e+00/0.00e+00   0.00e+00/0.00e+00   0.00e+00/0.00e+00
saturated     d_xyz        2.71e-08/6.67e-08   4.71e-08/2.28e-06   9.93e-08/5.29e-05   1.93e-07/5.34e-04
saturated     d_scaling    4.49e-08/5.51e-07   9.01e-08/1.16e-05   1.27e-07/1.18e-04   1.73e-07/5.44e-04
saturated     d_rotation   6.46e-08/5.99e-07   1.59e-07/1.23e-05   3.31e-07/1.48e-04   5.72e-07/3.42e-03
saturated     colour       3.02e-08/2.99e-08   1.10e-07/1.10e-07   1.92e-06/1.87e-06   3.99e-06/3.99e-06
saturated     d_cov3d      3.25e-07/3.19e-07   6.18e-06/6.02e-06   8.11e-05/1.02e-04   5.16e-04/6.80e-04
saturated     d_sh_rest    2.54e-06/2.54e-06   3.30e-02/3.30e-02   1.00e+00/1.00e+00   1.00e+00/1.00e+00

Forward tensors and the cov3d path's gradients track the fp32 statement
within a factor 1.5 at every quantile: both carry the same error, Sigma and
cov2d are fp32 and inv(cov2d) amplifies their rounding by cond(cov2d) (up to
2e4 here).  (saturated d_sh_rest: sigmoid(x) rounds to 1 for x > 17 in fp32, in
the kernel as in torch, so c (1 - c) is 0 where fp64 has 1e-13 times the
cotangent.)

The raw path's d_xyz, d_scaling and d_rotation sit one to four orders below
the statement since this test's first run.  Then the backward built Sigma and
the rotation in fp32 and read the conic back as fp32, d_scaling and d_rotation
tracked the statement (plain: 6.19e-07/5.84e-07 and 7.42e-07/6.12e-07 at the
median) and d_rotation's maximum missed the bound in 11 cases: 9.46e-03
against 4 x 2.31e-03 (plain), 3.44e-02 against 4 x 4.48e-03 (needles).  The
rows at the maximum are needles with two nearly equal thin axes; a rotation
matrix rounded to fp32 turns their axes by 1e-7 rad and their nearly cancelling
rotation gradient by 1e-2 of itself (found by restating the stages in torch at
mixed precision: only the quaternion's normalisation, R(q), Sigma, the conic
and Rq^T dS Rq in double together remove it).  k_project_bwd's raw path now
does that, in the Gaussian's own frame.
"""
import ctypes as C
import math

import numpy as np
import pytest
import torch

import golden_io as G
import project_reference as PR
from test_sh import _posed_view

W, H, FOVX = 160, 120, math.radians(60.0)
FOVY = 2 * math.atan(math.tan(FOVX / 2) * H / W)
QS = (50, 90, 99, 100)
FACTOR, FLOOR = 4.0, 1e-7
# A cull comparison within this relative distance of its boundary may round
# either way in fp32: ~20 operations of <= 0.5 ulp (6e-8) each on the way to
# mean, radius and Z.  Uniformly spread positions put ~1e-5 of a case there.
VIS_MARGIN = 1e-5
VIS_CAP = 0.005

POPULATIONS = ("plain", "needles", "quats", "near_behind", "posed", "radius_clamp", "saturated")
SIZES = {"plain": 4000, "needles": 3000, "quats": 2000, "near_behind": 3000, "posed": 3000, "radius_clamp": 3000,
         "saturated": 2000}
SMALL_N = (1, 255, 256, 257)


def camera(pop):
    return PR.make_camera(W, H, FOVX, FOVY, _posed_view().double().numpy() if pop == "posed" else None)


def population(pop, n):
    """fp32 parameter tensors of population `pop` (a prefix of one fixed draw
    per population, so that a small case is the large one's first rows)."""
    full = _population(pop)
    return {k: (None if v is None else v[:n].clone()) for k, v in full.items()}


_POPS: dict = {}


def _population(pop):
    if pop in _POPS:
        return _POPS[pop]
    n = SIZES[pop]
    rng = np.random.default_rng(100 + POPULATIONS.index(pop))
    tx, ty = math.tan(FOVX / 2), math.tan(FOVY / 2)
    z = rng.uniform(1, 6, n)
    u, v = rng.uniform(-1.15, 1.15, n), rng.uniform(-1.15, 1.15, n)  # a little past the image edge
    sig = np.exp(rng.uniform(math.log(0.002), math.log(0.3), (n, 3)))
    q = rng.standard_normal((n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    logits = rng.uniform(-2, 2, (n, 3))
    op_logit = rng.uniform(-3, 3, n)
    rest = 0.4 * rng.standard_normal((n, 15, 3))
    if pop == "needles":
        sig = np.exp(rng.uniform(math.log(0.002), math.log(0.03), (n, 3)))
        sig[np.arange(n), rng.integers(0, 3, n)] *= math.exp(2.5)
    elif pop == "quats":
        q *= np.exp(rng.uniform(math.log(0.03), math.log(30.0), (n, 1)))
    elif pop == "near_behind":
        k = n // 3
        z[:k] = rng.uniform(0.05, 0.3, k) * rng.choice([-1.0, 1.0], k)   # at the camera plane, both sides
        z[k:2 * k] = -rng.uniform(0.05, 6.0, k)                          # behind
        u[2 * k:] = rng.uniform(3, 20, n - 2 * k) * rng.choice([-1.0, 1.0], n - 2 * k)  # far off screen
        sig = np.exp(rng.uniform(math.log(0.002), math.log(0.05), (n, 3)))
    elif pop == "radius_clamp":
        k = n // 3
        sig[:k] = np.exp(rng.uniform(math.log(1e-6), math.log(1e-4), (k, 3)))  # r < radius_min
        sig[k:2 * k] = np.exp(rng.uniform(0.0, math.log(3.0), (k, 3)))         # r > radius_max
        # visible (mx < W + r) with an empty pixel rectangle: int(mx) = W, r = radius_min
        fx, cx = 0.5 * W / tx, 0.5 * W
        u[:8] = (W + 0.004 - cx) / fx / tx
    elif pop == "saturated":
        logits = rng.uniform(-30, 30, (n, 3))
        op_logit = rng.uniform(-30, 30, n)
    xc = np.stack([u * z * tx, v * z * ty, z], 1)
    if pop == "posed":
        wv = _posed_view().double().numpy()
        xc = (xc - wv[:3, 3]) @ wv[:3, :3]  # R^T (Xc - t)
    t = lambda a: torch.tensor(np.asarray(a, np.float32))
    d = dict(xyz=t(xc), scaling=t(np.log(sig)), rotation=t(q), color_logits=t(logits), opacity=t(op_logit), sh_rest=t(rest))
    # the covariance input of the cov3d cases: the fp64 statement's, rounded once (symmetric)
    cov = PR.covariance(d["scaling"].double(), d["rotation"].double())
    d["cov3d"] = (0.5 * (cov + cov.transpose(1, 2))).float()
    _POPS[pop] = d
    return d


# name -> (covariance input, sh_degree, opacity_is_logit, viewspace / conic cotangents)
CONFIGS = {
    "hot": ("raw", 0, True, False), "hot_prob": ("raw", 0, False, False), "raw_cot": ("raw", 0, True, True),
    "cov_cot": ("cov", 0, False, True), "raw_sh1": ("raw", 1, True, False), "raw_sh2": ("raw", 2, False, True),
    "raw_sh3": ("raw", 3, True, False), "cov_sh1": ("cov", 1, False, False), "cov_sh2": ("cov", 2, True, False),
    "cov_sh3": ("cov", 3, False, True),
}


def case_inputs(pop, n, config):
    kind, deg, logit, _ = CONFIGS[config]
    d = population(pop, n)
    if kind == "raw":
        d["cov3d"] = None
    else:
        d["scaling"] = d["rotation"] = None
    if not logit:
        d["opacity"] = torch.sigmoid(d["opacity"].double()).float()
    if deg == 0:
        d["sh_rest"] = None
    return d, deg, logit


def cotangents(pop, n, config):
    """acc [n,10] (the grad_sums layout), g_means2d, g_conics; every 16th
    row all zero (the kernel's early return), the following one zero but for
    opacity and colour."""
    rng = np.random.default_rng(7 + n)
    acc = rng.uniform(-1, 1, (n, 10))
    gm, gc = rng.uniform(-1, 1, (n, 2)), rng.uniform(-1, 1, (n, 4))
    acc[0::16] = 0
    gm[0::16] = 0
    gc[0::16] = 0
    acc[1::16, [0, 1, 2, 3, 4, 9]] = 0
    gm[1::16] = 0
    gc[1::16] = 0
    t = lambda a: torch.tensor(a.astype(np.float32))
    return (t(acc), t(gm), t(gc)) if CONFIGS[config][3] else (t(acc), None, None)


def row_rel(d, d64, what):
    """Row-relative errors of the rows whose fp64 value is not all zero; the others must be exact zeros."""
    d64 = np.asarray(d64, np.float64)
    d = np.asarray(d, np.float64).reshape(d64.shape[0], -1)
    d64 = d64.reshape(d64.shape[0], -1)
    den = np.abs(d64).max(1)
    zero = den == 0
    assert not d[zero].any(), f"{what}: a row that is zero in fp64 is not zero"
    with np.errstate(invalid="ignore"):
        e = np.abs(d - d64).max(1)[~zero] / den[~zero]
    return e


def yardstick(stmt32, ref64, name=""):
    """The fp32 statement's row-relative errors (a non-finite row counts as infinitely wrong)."""
    with np.errstate(invalid="ignore"):
        return np.nan_to_num(row_rel(np.nan_to_num(stmt32, nan=np.inf), ref64, name + " (fp32 statement)"),
                             nan=np.inf, posinf=np.inf)


def quantile_errors(name, kern, stmt32, ref64, rows=None):
    """Failure strings of the quantile rule (module docstring); prints the measured pairs."""
    sel = (lambda a: np.asarray(a)[rows]) if rows is not None else np.asarray
    assert np.isfinite(sel(kern)).all(), f"{name}: non-finite kernel output"
    return quantile_rule(name, row_rel(sel(kern), sel(ref64), name), yardstick(sel(stmt32), sel(ref64), name))


def quantile_rule(name, ek, es):
    if ek.size == 0:
        return []
    qk, qs = np.percentile(ek, QS), np.percentile(es, QS)
    print(f"  {name:>22}: kernel / fp32 statement  " +
          "  ".join(f"p{q}: {a:.2e} / {b:.2e}" for q, a, b in zip(QS, qk, qs)))
    return [f"{name} p{q}: kernel {a:.3e} > {FACTOR} x {b:.3e} + {FLOOR}" for q, a, b in zip(QS, qk, qs)
            if not a <= FACTOR * b + FLOOR]


def vis_flips(name, vis, ref):
    """Rows whose visibility differs from the fp64 decision; all must be
    within rounding of a cull boundary (each printed), at most VIS_CAP of the case."""
    vis = np.asarray(vis, bool)
    flip = np.nonzero(vis != ref["vis"].numpy())[0]
    margin = ref["margin"].numpy()
    for g in flip:
        print(f"  {name}: vis differs at Gaussian {g}: margin {margin[g]:.3e}, mean {ref['means2d'][g].tolist()}, "
              f"radius {float(ref['radii'][g]):.6g}, Z {float(ref['Z'][g]):.6g}")
    assert (margin[flip] < VIS_MARGIN).all(), f"{name}: visibility differs away from a cull boundary"
    assert len(flip) <= VIS_CAP * len(vis), f"{name}: {len(flip)} of {len(vis)} visibility decisions differ"
    return flip


# ------------------------------------------------------------------ CPU ----
def _oracle_scene(d, cam_kw=None):
    o = G.oracle()
    n = d["xyz"].shape[0]
    return o.Scene(xyz=d["xyz"].numpy(), cov3d=d["cov3d"].numpy(), color_logits=d["color_logits"].numpy(),
                   opacity=np.full(n, 0.5, np.float32), wv=np.eye(4), width=W, height=H, fovx=FOVX, fovy=FOVY,
                   bg=np.zeros(3, np.float32))


def test_statement_matches_oracle_forward():
    d, deg, logit = case_inputs("plain", 600, "cov_cot")
    ref = PR.forward(camera("plain"), d)
    o = G.oracle().render_forward(_oracle_scene(d))
    flip = vis_flips("oracle", o["vis"], ref)
    assert len(flip) == 0
    out = dict(means2d=ref["means2d"].numpy(), radii=ref["radii"].numpy(), conics=ref["conics"].numpy(), vis=ref["vis"].numpy())
    assert not G.check_projection(out, o)
    # and per Gaussian: the oracle's fp32 rows within fp32 rounding of the fp64 ones
    for k in ("means2d", "conics", "radii"):
        e = row_rel(o[k], ref[k].numpy(), k)
        assert np.median(e) <= 1e-6 and e.max() <= 1e-3, (k, np.median(e), e.max())


def test_statement_matches_oracle_projection_backward():
    """Zero pixel cotangents, random cotangents on means2d and conics: the
    oracle's projection backward (d_xyz, d_cov3d) alone."""
    n = 600
    d, deg, logit = case_inputs("plain", n, "cov_cot")
    acc, gm, gc = cotangents("plain", n, "cov_cot")
    z = np.zeros((H, W), np.float32)
    o = G.oracle().render_backward(_oracle_scene(d), np.zeros((3, H, W), np.float32), z, z, gm.numpy(), gc.numpy())
    ref = PR.backward(camera("plain"), d, torch.zeros(n, 10), gm, gc)
    errs = G.check_grad("xyz", o["grads"]["xyz"], ref["xyz"].numpy()) + \
        G.check_grad("cov3d", o["grads"]["cov3d"], ref["cov3d"].numpy())
    assert not errs, errs
    for k in ("xyz", "cov3d"):
        e = row_rel(o["grads"][k], ref[k].numpy(), k)
        assert np.median(e) <= 1e-5, (k, np.median(e))


@pytest.mark.parametrize("config", ["raw_cot", "cov_sh3", "raw_sh2"])
def test_statement_matches_finite_differences(config):
    """Central differences of the per-Gaussian terms L_g of L in fp64, step
    h = 1e-6 (of a covariance's smallest eigenvalue).  Truncation is h^2 / 6 times L_g's third derivative, below 1e-8
    of a gradient row on the plain population (depths >= 1, pixel sigmas >=
    0.03): bound 1e-6 of the row.  Rounding is that of L_g's two evaluations
    over 2 h, a few eps64 of the sum of L_g's terms in magnitude (the conic
    terms reach 1e5 where the opacity term is 0.1): bound 16 eps64 sum|terms| / h."""
    n = 200
    cam = camera("plain")
    d, deg, logit = case_inputs("plain", n, config)
    acc, gm, gc = cotangents("plain", n, config)
    grads = PR.backward(cam, d, acc, gm, gc, sh_degree=deg, opacity_is_logit=logit)
    base = PR.cast_inputs(d, torch.float64)
    if deg == 0:
        base.pop("sh_rest", None)
    cot = [None if t is None else t.double() for t in (acc, gm, gc)]

    def terms(p):
        with torch.no_grad():
            return PR.blend_scalar(PR.project(cam, sh_degree=deg, opacity_is_logit=logit, **p), *cot)
    with torch.no_grad():
        out = PR.project(cam, sh_degree=deg, opacity_is_logit=logit, **base)
        mag = PR.blend_scalar({k: v.abs() for k, v in out.items() if v.dtype == torch.float64},
                              *[None if t is None else t.abs() for t in cot])
    for name, t in base.items():
        flat = t.reshape(n, -1)
        fd = torch.empty_like(flat)
        # (a covariance's own scale is its smallest eigenvalue: the step relative to it)
        h = 1e-6 * (torch.linalg.eigvalsh(t).min(-1).values if name == "cov3d" else torch.ones(n, dtype=torch.float64))
        for k in range(flat.shape[1]):
            e = torch.zeros_like(flat)
            e[:, k] = h
            hi, lo = dict(base), dict(base)
            hi[name], lo[name] = (flat + e).reshape(t.shape), (flat - e).reshape(t.shape)
            fd[:, k] = (terms(hi) - terms(lo)) / (2 * h)
        g = grads[name].reshape(n, -1)
        if deg and name == "sh_rest":
            nb = (deg + 1) ** 2 - 1
            assert not g.reshape(n, 15, 3)[:, nb:].any()
        tol = (1e-6 * g.abs().max(1).values + 16 * torch.finfo(torch.float64).eps * mag / h).clamp_min(1e-300)
        err = (fd - g).abs().max(1).values
        print(f"  {name}: max err / bound {(err / tol).max().item():.3g}")
        assert g.abs().max().item() > 0 and bool((err <= tol).all()), (name, (err / tol).max().item())


@pytest.mark.parametrize("pop", POPULATIONS)
def test_fp32_statement_visibility_recipe(pop):
    """The exemption recipe on the CPU: the fp32 statement's visibility against
    the fp64 one flips only within VIS_MARGIN of a cull boundary."""
    cam = camera(pop)
    d, deg, logit = case_inputs(pop, SIZES[pop], "hot")
    ref, f32 = PR.forward(cam, d), PR.forward(cam, d, torch.float32)
    vis_flips(pop, f32["vis"].numpy(), ref)
    assert ref["vis"].any() and not ref["vis"].all()


# ------------------------------------------------------------------ GPU ----
_REFS: dict = {}   # (pop, n, config) -> fp64 / fp32 statement forward and backward
_FWD: dict = {}    # (pop, n, config) -> the kernel's forward


def references(pop, n, config):
    key = (pop, n, config)
    if key not in _REFS:
        cam = camera(pop)
        d, deg, logit = case_inputs(pop, n, config)
        cot = cotangents(pop, n, config)
        r = {}
        for name, dt in (("f64", torch.float64), ("f32", torch.float32)):
            r[name] = dict(fwd=PR.forward(cam, d, dt, deg, logit), bwd=PR.backward(cam, d, *cot, dt, deg, logit))
        _REFS[key] = r
    return _REFS[key]


GUARD = 64


def _guarded(rows, cols, dtype, fill, dev):
    """[rows + GUARD, cols] filled with `fill`: the kernel may write the first `rows` only."""
    return torch.full((rows + GUARD, cols) if cols else (rows + GUARD,), fill, dtype=dtype, device=dev)


def _guard_intact(t, rows, fill):
    tail = t[rows:]
    return bool(torch.isnan(tail).all()) if isinstance(fill, float) and math.isnan(fill) else bool((tail == fill).all())


def _structs(pkg, cuda, pop, d, deg, logit):
    RZ = pkg.rasterizer
    c = camera(pop)
    cam = RZ.CameraParams(c.width, c.height, c.fx, c.fy, c.cx, c.cy, c.view, (0.0, 0.0, 0.0), c.radius_min,
                          c.radius_max, c.tile_size)
    dd = {k: (None if v is None else v.to(cuda).contiguous()) for k, v in d.items()}
    n = d["xyz"].shape[0]
    gst = RZ._build_gaussians_struct(n, dd["xyz"], dd["cov3d"], dd["scaling"], dd["rotation"], dd["color_logits"],
                                     dd["opacity"], logit, dd["sh_rest"], deg)
    return cam.to_struct(), gst, dd


def gpu_forward(pkg, cuda, pop, n, config, key_bits=32, key_base=0, cache=True):
    key = (pop, n, config)
    if cache and key in _FWD:
        return _FWD[key]
    N = pkg._native
    lib = N.load()
    d, deg, logit = case_inputs(pop, n, config)
    cs, gst, dd = _structs(pkg, cuda, pop, d, deg, logit)
    nan = float("nan")
    nblk = (n + 255) // 256
    o = dict(means2d=_guarded(n, 2, torch.float32, nan, cuda), conics=_guarded(n, 4, torch.float32, nan, cuda),
             radii=_guarded(n, 0, torch.float32, nan, cuda), vis=_guarded(n, 0, torch.uint8, 7, cuda),
             records=_guarded(n, 12, torch.float32, nan, cuda), rects=_guarded(n, 2, torch.int32, -7, cuda),
             depth_keys=_guarded(n, 0, torch.int32, -7, cuda), key_minmax=_guarded(2 * nblk, 0, torch.int32, -7, cuda))
    a = N.GsProjectArgs(cs, gst, *(N.ptr(o[k]) for k in ("means2d", "conics", "radii", "vis", "records", "rects",
                                                          "depth_keys")), key_base, key_bits, N.ptr(o["key_minmax"]))
    N.check(lib.gs_project_forward(C.byref(a), torch.cuda.current_stream().cuda_stream), "gs_project_forward")
    torch.cuda.synchronize()
    fills = dict(means2d=nan, conics=nan, radii=nan, vis=7, records=nan, rects=-7, depth_keys=-7, key_minmax=-7)
    for k, t in o.items():
        rows = 2 * nblk if k == "key_minmax" else n
        assert _guard_intact(t, rows, fills[k]), f"{k}: written past row {rows}"
    res = {k: t[:(2 * nblk if k == "key_minmax" else n)] for k, t in o.items()}
    res["_inputs"] = dd
    res["_structs"] = (cs, gst)
    if cache:
        _FWD[key] = res
    return res


def expected_integers(m2, r, z, vis, key_bits=32, key_base=0, T=16):
    """rects, record word 11, depth keys and the per-block key range, from the
    kernel's own fp32 means2d, radii, Z and vis."""
    n = len(r)
    m2 = np.where(vis[:, None], m2, 0).astype(np.float64)
    ri = np.trunc(np.where(vis, r, 0)).astype(np.int64)      # int(): toward zero
    icx, icy = np.trunc(m2[:, 0]).astype(np.int64), np.trunc(m2[:, 1]).astype(np.int64)
    x0, x1 = np.maximum(icx - ri, 0), np.minimum(icx + 1 + ri, W)
    y0, y1 = np.maximum(icy - ri, 0), np.minimum(icy + 1 + ri, H)
    ok = vis & (x0 < x1) & (y0 < y1)
    x0, x1, y0, y1 = (np.where(ok, v, 1) for v in (x0, x1, y0, y1))
    rects = np.stack([np.where(ok, (x0 // T) | (((x1 - 1) // T) << 16), 1),
                      np.where(ok, (y0 // T) | (((y1 - 1) // T) << 16), 1)], 1).astype(np.uint32)
    word11 = np.where(ok, (x0 // T) | ((y0 // T) << 12) | ((((x1 - 1) // T) - x0 // T) << 24), 0).astype(np.uint32)
    zbits = z.astype(np.float32).view(np.uint32)
    mask = np.uint32(0xFFFFFFFF if key_bits >= 32 else (1 << key_bits) - 1)
    keys = np.where(vis, (zbits - np.uint32(key_base)) & mask, mask).astype(np.uint32)
    nblk = (n + 255) // 256
    mm = np.empty(2 * nblk, np.uint32)
    for b in range(nblk):
        zb = zbits[256 * b:256 * (b + 1)][vis[256 * b:256 * (b + 1)]]
        mm[2 * b], mm[2 * b + 1] = (zb.min(), zb.max()) if zb.size else (0xFFFFFFFF, 0)
    return rects, word11, keys, mm, ok


def _cases(configs, small_configs):
    """Every population at its full size with every configuration; the sizes
    around a workgroup with one configuration per kernel instantiation."""
    return [(p, SIZES[p], c) for p in POPULATIONS for c in configs] + \
        [(p, n, c) for p in POPULATIONS for n in SMALL_N for c in small_configs]


@pytest.mark.gpu
@pytest.mark.parametrize("pop,n,config", _cases(["hot", "hot_prob", "raw_sh2", "cov_cot", "cov_sh3"], ["hot", "cov_sh3"]))
def test_project_forward(pkg, cuda, pop, n, config):
    out = gpu_forward(pkg, cuda, pop, n, config)
    ref = references(pop, n, config)
    r64, r32 = ref["f64"]["fwd"], ref["f32"]["fwd"]
    name = f"{pop}[{n}] {config}"
    print(name)
    cpu = {k: v.cpu().numpy() for k, v in out.items() if not k.startswith("_")}
    vis = cpu["vis"].astype(bool)
    assert set(np.unique(cpu["vis"])) <= {0, 1}
    vis_flips(name, vis, r64)
    errs = []
    for k in ("means2d", "conics", "radii"):
        errs += quantile_errors(k, cpu[k], r32[k].numpy().reshape(n, -1), r64[k].numpy().reshape(n, -1))
    both = vis & r64["vis"].numpy()
    rec = cpu["records"]
    if both.any():
        errs += quantile_errors("colour", rec[:, 6:9], r32["color"].numpy(), r64["color"].numpy(), both)
        errs += quantile_errors("opacity", rec[:, 5:6], r32["opacity"].numpy()[:, None], r64["opacity"].numpy()[:, None], both)
        errs += quantile_errors("Z", rec[:, 9:10], r32["Z"].numpy()[:, None], r64["Z"].numpy()[:, None], both)
    assert not errs, errs
    # the record repeats the outputs bit for bit
    assert np.array_equal(rec[vis][:, [0, 1, 2, 3]], np.concatenate([cpu["means2d"], cpu["conics"][:, [0, 3]]], 1)[vis])
    assert np.array_equal(rec[vis][:, 4], (cpu["conics"][:, 1] + cpu["conics"][:, 2])[vis])
    assert not rec[vis][:, 10].any()
    # integer work, exact, from the kernel's own floats
    z = np.where(vis, rec[:, 9], 1.0).astype(np.float32)
    rects, word11, keys, mm, ok = expected_integers(cpu["means2d"], cpu["radii"], z, vis)
    assert np.array_equal(cpu["rects"].view(np.uint32), rects)
    assert np.array_equal(rec[vis][:, 11].view(np.uint32), word11[vis])
    assert np.array_equal(cpu["depth_keys"].view(np.uint32), keys)
    assert np.array_equal(cpu["key_minmax"].view(np.uint32), mm)
    if pop == "radius_clamp" and n == SIZES[pop]:
        c = camera(pop)
        assert (cpu["radii"] == np.float32(c.radius_min)).sum() > 100 and (cpu["radii"] == np.float32(c.radius_max)).sum() > 100
        assert (vis & ~ok).any(), "a visible Gaussian with an empty rectangle"
    if pop == "near_behind" and n == SIZES[pop]:
        assert (~vis).sum() > n // 3 and vis.any()
    # a 20-bit depth window with a base: the same floats, other keys
    base = int(np.float32(0.75).view(np.uint32))
    win = gpu_forward(pkg, cuda, pop, n, config, key_bits=20, key_base=base, cache=False)
    for k in ("means2d", "conics", "radii", "vis", "rects", "key_minmax"):
        assert torch.equal(win[k], out[k]), k
    keys20 = expected_integers(cpu["means2d"], cpu["radii"], z, vis, 20, base)[2]
    assert np.array_equal(win["depth_keys"].cpu().numpy().view(np.uint32), keys20)


def gpu_backward(pkg, cuda, pop, n, config, order=None, drop_cotangents=False):
    """gs_project_backward with pair_grads = NULL and acc as grad_sums; the
    forward's means2d / conics / vis; dummy rectangles and slot offsets."""
    N = pkg._native
    lib = N.load()
    kind, deg, logit, _ = CONFIGS[config]
    fwd = gpu_forward(pkg, cuda, pop, n, config)
    cs, gst = fwd["_structs"]
    acc, gm, gc = (None if t is None else t.to(cuda) for t in cotangents(pop, n, config))
    if drop_cotangents:
        gm = gc = None
    nan = float("nan")
    raw = kind == "raw"
    o = dict(d_xyz=_guarded(n, 3, torch.float32, nan, cuda), d_color_logits=_guarded(n, 3, torch.float32, nan, cuda),
             d_opacity=_guarded(n, 0, torch.float32, nan, cuda))
    if raw:
        o.update(d_scaling=_guarded(n, 3, torch.float32, nan, cuda), d_rotation=_guarded(n, 4, torch.float32, nan, cuda))
    else:
        o["d_cov3d"] = _guarded(n, 9, torch.float32, nan, cuda)
    if deg:
        o["d_sh_rest"] = _guarded(n, 45, torch.float32, nan, cuda)
    rects = torch.zeros((n, 2), dtype=torch.int32, device=cuda)
    pair_offset = torch.zeros((n,), dtype=torch.int32, device=cuda)
    od = None if order is None else torch.tensor(np.asarray(order, np.int32), device=cuda)
    a = N.GsProjectBwdArgs(cs, gst, N.ptr(fwd["means2d"]), N.ptr(fwd["conics"]), N.ptr(fwd["vis"]), N.ptr(rects),
                           N.ptr(pair_offset), N.ptr(od), None, N.ptr(gm), N.ptr(gc), N.ptr(o["d_xyz"]),
                           N.ptr(o.get("d_cov3d")), N.ptr(o.get("d_scaling")), N.ptr(o.get("d_rotation")),
                           N.ptr(o["d_color_logits"]), N.ptr(o["d_opacity"]), N.ptr(o.get("d_sh_rest")), None,
                           N.ptr(acc), 0)
    N.check(lib.gs_project_backward(C.byref(a), torch.cuda.current_stream().cuda_stream), "gs_project_backward")
    torch.cuda.synchronize()
    for k, t in o.items():
        assert _guard_intact(t, n, nan), f"{k}: written past row {n}"
    return {k: t[:n].cpu().numpy() for k, t in o.items()}


GRAD_OF = dict(d_xyz="xyz", d_color_logits="color_logits", d_opacity="opacity", d_scaling="scaling",
               d_rotation="rotation", d_cov3d="cov3d", d_sh_rest="sh_rest")


@pytest.mark.gpu
@pytest.mark.parametrize("pop,n,config", _cases(list(CONFIGS), ["hot", "raw_cot", "cov_sh3"]))
def test_project_backward(pkg, cuda, pop, n, config):
    """Every gradient tensor by the quantile rule; zeros exact; `order` bit for bit."""
    kind, deg, logit, cot = CONFIGS[config]
    got = gpu_backward(pkg, cuda, pop, n, config)
    ref = references(pop, n, config)
    r64, r32 = ref["f64"]["bwd"], ref["f32"]["bwd"]
    name = f"{pop}[{n}] {config}"
    print(name)
    errs = []
    for k, v in got.items():
        p = GRAD_OF[k]
        errs += quantile_errors(k, v.reshape(n, -1), r32[p].numpy().reshape(n, -1), r64[p].numpy().reshape(n, -1))
    if deg:
        nb = (deg + 1) ** 2 - 1
        assert not got["d_sh_rest"].reshape(n, 15, 3)[:, nb:].any(), "d_sh_rest past the degree"
    # rows of all-zero cotangents: exact zeros but for the SH term of d_xyz (row_rel checks them
    # against fp64 zeros; here that the case has such rows)
    assert n < 17 or not np.any(r64["scaling" if kind == "raw" else "cov3d"].numpy()[0::16])
    # order: a permuted walk writes the same bits (the quantile rule's findings are raised after it)
    perm = np.random.default_rng(n).permutation(n)
    walked = gpu_backward(pkg, cuda, pop, n, config, order=perm)
    if not cot and deg == 0 and kind == "raw":
        # the same inputs through the hot instantiation (above) and the generic one (order given)
        same = all(np.array_equal(walked[k], got[k]) for k in got)
        print(f"  hot and generic instantiation bit-equal: {same}")
        for k in got:  # to rounding: their difference by the rule their errors are held to
            p = GRAD_OF[k]
            bad = quantile_rule(k + " hot - generic", row_rel(walked[k], got[k].reshape(n, -1), k),
                                yardstick(r32[p].numpy().reshape(n, -1), r64[p].numpy().reshape(n, -1)))
            assert not bad, bad
        ident = gpu_backward(pkg, cuda, pop, n, config, order=np.arange(n))
        for k in got:
            assert np.array_equal(walked[k], ident[k]), f"{k}: order changes the result"
    else:
        for k in got:
            assert np.array_equal(walked[k], got[k]), f"{k}: order changes the result"
    assert not errs, errs
