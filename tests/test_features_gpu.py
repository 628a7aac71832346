"""Per-Gaussian feature channels through the blend (render(..., features=F)):
the colour outputs stay bit for bit, the feature pass replays the colour
pass's decisions, and its forward and gradients match the reference's golden
gradients (zero-background fixtures, features = sigmoid(logits)) and the
pinned oracle (any C, any range).

Tolerances are tests/golden_io.py's: IMG_ATOL on pixel values (scaled by the
feature range where an affine map is applied), check_grad's
1e-4 max|d_ref| + 1e-7 per gradient tensor."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import features_util as U
import golden_io as G
from stubs import Gauss

pytestmark = pytest.mark.gpu

OUTPUTS = ("image", "alpha", "depth", "viewspace_points", "conics", "radii", "visibility_filter")


def _colour_loss(out, f, dev):
    return sum((out[k] * U.tensor(f["g_" + k], dev)).sum() for k in ("image", "alpha", "depth"))


# ---- 1. colour outputs untouched ---------------------------------------------
@pytest.mark.parametrize("name", ["model_random", "random_bg", "tile12"])
def test_colour_outputs_and_gradients_untouched(pkg, cuda, name):
    f = G.load(name)
    n = f["xyz"].shape[0]
    F = torch.rand((n, 5), generator=torch.Generator().manual_seed(3)).to(cuda).requires_grad_()
    res = []
    for feats in (None, F):
        m, leaves, _ = U.gaussians_of(pkg, cuda, f)
        _, out = U.render(pkg, cuda, f, feats, model=m)
        _colour_loss(out, f, cuda).backward()
        res.append((out, leaves))
    (a, la), (b, lb) = res
    assert "features" not in a and b["features"].shape == (5, int(f["height"]), int(f["width"]))
    assert b["features"].dtype == torch.float32
    for k in OUTPUTS:
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    for k in la:
        assert la[k].grad is not None and torch.equal(la[k].grad, lb[k].grad), k
    assert F.grad is None  # (the feature image took no part in the loss)


# ---- 2. the decisions are the colour pass's ---------------------------------
@pytest.mark.parametrize("name", ["saturate", "radius_clamp", "offscreen", "tile8", "tile32", "radius80_tile8"])
def test_decisions_are_the_colour_pass(pkg, cuda, name):
    f = G.load(name)
    n = f["xyz"].shape[0]
    _, out = U.render(pkg, cuda, f, torch.ones((n, 1), device=cuda))
    alpha, ones = out["alpha"][0], out["features"][0]
    below = alpha < 1
    assert below.any()
    assert torch.equal(ones[below], alpha[below])  # sum_i c_i is A, the same additions in the same order
    if name == "saturate":
        assert (alpha >= 0.995).any(), "the termination is exercised"
    z = U.camera_depths(f)
    _, out = U.render(pkg, cuda, f, U.tensor(z, cuda).reshape(n, 1))
    want = out["depth"][0].detach().double() * (out["alpha"][0].detach().double() + 1e-6)  # depth = D / (A + 1e-6)
    err = float((out["features"][0].detach().double() - want).abs().max())
    print(f"  {name}: max |sum c Z - depth (alpha + 1e-6)| = {err:.3g} (max Z {z.max():.3g})")
    assert err <= 1e-4 * float(np.abs(z).max())


# ---- 3. against the reference's own gradients --------------------------------
ZERO_BG = [n for n in G.fixture_names() if "g_image" in G.load(n) and not np.any(G.load(n)["bg"])]


def test_enough_zero_background_fixtures():
    assert len(ZERO_BG) >= 6, ZERO_BG
    assert any("scaling" in G.load(n) for n in ZERO_BG), "the raw covariance path is covered"


@pytest.mark.parametrize("name", ZERO_BG)
def test_reference_gradients_through_features(pkg, cuda, name):
    """bg = 0: the reference's image is sum_i c_i sigmoid(logit_i), unclamped,
    so features = sigmoid(logits) (a torch node) must reproduce its image and,
    with its image cotangent on the feature output, its gradients."""
    f = G.load(name)
    n = f["xyz"].shape[0]
    m, leaves, logits = U.gaussians_of(pkg, cuda, f)
    _, out = U.render(pkg, cuda, f, torch.sigmoid(logits), model=m)
    err = G.max_err(U.np_(out["features"]), f["image"])
    print(f"  {name}: features vs reference image: max err {err:.3g}")
    errs = [] if err <= G.IMG_ATOL else [f"features: max abs err {err:.3g}"]
    L = (out["features"] * U.tensor(f["g_image"], cuda)).sum() + (out["alpha"] * U.tensor(f["g_alpha"], cuda)).sum() \
        + (out["depth"] * U.tensor(f["g_depth"], cuda)).sum()
    L.backward()
    for k, t in leaves.items():
        errs += G.check_grad(k, U.leaf_grad(k, t, n), f["d_" + k])
    assert not errs, errs


# ---- 4. any C, any range, against the pinned oracle --------------------------
_ORACLE_CASES: dict = {}


def _oracle_case(pkg, cuda, name, c):
    key = (name, c)
    if key not in _ORACLE_CASES:
        f = G.load(name)
        got = U.feature_case(pkg, cuda, f, c, seed=100 + c)
        exp, grads, edge = U.oracle_features(f, got["f01"], got["a"], got["b"], got["gF"])
        _ORACLE_CASES[key] = (got, exp, grads, edge)
    return _ORACLE_CASES[key]


@pytest.mark.parametrize("c", [1, 4, 5, 9])
@pytest.mark.parametrize("name", ["model_random", "tile8", "tile12", "tile32", "posed_camera"])
def test_any_channels_any_range_vs_oracle(pkg, cuda, name, c):
    got, exp, grads, edge = _oracle_case(pkg, cuda, name, c)
    assert not edge.any(), f"{name}: {int(edge.sum())} knife-edge pixels -- the wrong scene for this test"
    tol = G.IMG_ATOL * float(np.max(np.abs(got["a"]) + np.abs(got["b"])))
    err = G.max_err(got["features"], exp)
    print(f"  {name} C={c}: features max err {err:.3g} (tol {tol:.3g})")
    errs = [] if err <= tol else [f"features: max abs err {err:.3g} > {tol:.3g}"]
    errs += G.check_grad("features", got["d_features"], grads["features"])
    errs += G.check_grad("xyz", got["d_xyz"], grads["xyz"])
    errs += G.check_grad("cov3d", got["d_cov3d"], grads["cov3d"])
    errs += G.check_grad("opacity", got["d_opacity"], grads["opacity"])
    assert not errs, errs


# ---- 5. sub-pixel Gaussian ---------------------------------------------------
def test_sub_pixel_gaussian(pkg, cuda):
    """One Gaussian with sigma_y = 0.05 px (sigma_x = 0.3 px) inside one 8x8
    cell: the dy^2 row moment must be taken about the row nearest the mean
    (about the cell's row 0 it cancels to ~1e-4 of the gradient's scale).
    The conic gradient is compared where it is observable, in d_cov3d (and
    d_xyz, d_opacity), with the oracle route of the test above."""
    W = H = 32
    fov = np.radians(60.0)
    fpx = 0.5 * W / np.tan(fov / 2)
    mean_px = np.array([12.2, 11.1])
    f = dict(xyz=np.array([[(mean_px[0] - 16) / fpx, -(mean_px[1] - 16) / fpx, 1.0]], np.float32),
             cov3d=np.diag([(0.3 / fpx) ** 2, (0.05 / fpx) ** 2, 1e-8]).astype(np.float32)[None],
             color_logits=np.zeros((1, 3), np.float32), opacity=np.array([0.7], np.float32),
             wv=np.eye(4, dtype=np.float32), width=W, height=H, cam_width=W, cam_height=H, fovx=fov, fovy=fov,
             bg=np.zeros(3, np.float32))
    got = U.feature_case(pkg, cuda, f, 2, seed=55)
    g = Gauss(f["xyz"], f["cov3d"], f["color_logits"], f["opacity"], cuda)
    _, out = U.render(pkg, cuda, f, model=g)
    m2, q = U.np_(out["viewspace_points"])[0], U.np_(out["conics"])[0]
    cov2 = np.linalg.inv(q.astype(np.float64))
    assert abs(np.sqrt(cov2[1, 1]) - 0.05) < 0.01 and 8 < m2[0] < 15 and 8 < m2[1] < 15, (m2, cov2)
    assert np.count_nonzero(got["features"][0]) >= 2, "the Gaussian reaches pixels"
    exp, grads, edge = U.oracle_features(f, got["f01"], got["a"], got["b"], got["gF"])
    assert not edge.any()
    errs = G.check_grad("cov3d", got["d_cov3d"], grads["cov3d"])
    errs += G.check_grad("xyz", got["d_xyz"], grads["xyz"])
    errs += G.check_grad("opacity", got["d_opacity"], grads["opacity"])
    errs += G.check_grad("features", got["d_features"], grads["features"])
    assert not errs, errs


# ---- 6. determinism and second backward --------------------------------------
@pytest.mark.parametrize("name", ["zero_bg_random", "tile12"])
def test_deterministic_and_second_backward(pkg, cuda, name):
    f = G.load(name)
    keys = ("features", "d_features", "d_xyz", "d_cov3d", "d_opacity")
    r1, r2 = (U.feature_case(pkg, cuda, f, 6, seed=7) for _ in range(2))
    for k in keys:
        assert np.array_equal(r1[k], r2[k]), k
    n = f["xyz"].shape[0]
    g = Gauss(f["xyz"], f["cov3d"], f["color_logits"], f["opacity"], cuda)
    F = U.tensor(r1["a"] * r1["f01"] + r1["b"], cuda, grad=True)
    _, out = U.render(pkg, cuda, f, F, model=g)
    # both outputs in the loss: the colour pass's flags and the feature pass's are both reused
    L = (out["features"] * U.tensor(r1["gF"], cuda)).sum() + _colour_loss(out, f, cuda)
    leaves = (F, g.xyz, g.cov, g.op, g.feats)
    first = torch.autograd.grad(L, leaves, retain_graph=True)
    second = torch.autograd.grad(L, leaves)
    for x, y in zip(first, second):
        assert torch.equal(x, y)
    assert first[0].shape == (n, 6)


# ---- 7. cell batches ---------------------------------------------------------
def test_cell_batches(pkg, cuda, tmp_path):
    """tile32's 16 cells in several batches (GS_PARTIAL_BUDGET, read at import:
    a child process) equal the one-batch result within check_grad, and each is
    bitwise reproducible."""
    f = G.load("tile32")
    keys = ("features", "d_features", "d_xyz", "d_cov3d", "d_opacity")
    one, again = (U.feature_case(pkg, cuda, f, 5, seed=9) for _ in range(2))
    for k in keys:
        assert np.array_equal(one[k], again[k]), k
    T = int(pkg.rasterizer._T_SEEN[cuda])
    assert pkg.rasterizer.cell_batch(16, T) == 16
    path = str(tmp_path / "batched.npz")
    env = dict(os.environ, GS_PARTIAL_BUDGET=str(41 * T * 5 + 1))  # 5 cells per batch: 5 + 5 + 5 + 1
    subprocess.run([sys.executable, os.path.join(G.ROOT, "tests", "features_util.py"), "tile32", "5", "9", path],
                   check=True, env=env, timeout=300)
    b = np.load(path)
    assert int(b["batch"]) == 5 and bool(b["same"])
    assert np.array_equal(b["features"], one["features"])  # (the forward does not batch)
    errs = []
    for k in keys[1:]:
        errs += G.check_grad(k, b[k], one[k])
    assert not errs, errs


def test_without_liveness_bitmap(pkg, cuda, monkeypatch):
    """live_bits == NULL (the forward's bitmap over its memory budget): every
    entry of a cell's evaluated prefix is replayed; the entries the bitmap
    would have passed over add exact zeros, so nothing changes, bit for bit."""
    f = G.load("tile32")
    keys = ("features", "d_features", "d_xyz", "d_cov3d", "d_opacity")
    with_bitmap = U.feature_case(pkg, cuda, f, 5, seed=9)
    monkeypatch.setattr(pkg.rasterizer, "LIVE_BUDGET_BYTES", 0)
    assert pkg.rasterizer.live_bitmap_bytes(pkg._native.load(), 16, 1000, 6) == 0
    without = U.feature_case(pkg, cuda, f, 5, seed=9)
    for k in keys:
        assert np.array_equal(with_bitmap[k], without[k]), k


# ---- 8. empty and partial frames ---------------------------------------------
def test_empty_frame(pkg, cuda):
    f = G.load("all_behind")
    g = Gauss(f["xyz"], f["cov3d"], f["color_logits"], f["opacity"], cuda)
    F = torch.ones((2, 3), device=cuda, requires_grad=True)
    _, out = U.render(pkg, cuda, f, F, model=g)
    assert out["features"].shape == (3, 64, 64) and not out["features"].any()
    (out["features"].sum() + out["alpha"].sum()).backward()
    assert F.grad.shape == (2, 3) and not F.grad.any()
    assert g.xyz.grad.shape == (2, 3) and not g.xyz.grad.any()
    assert g.cov.grad.shape == (2, 3, 3) and not g.cov.grad.any()


def test_culled_gaussians_get_zero_rows(pkg, cuda):
    f = G.load("offscreen")
    n = f["xyz"].shape[0]
    F = torch.ones((n, 3), device=cuda, requires_grad=True)
    _, out = U.render(pkg, cuda, f, F)
    out["features"].sum().backward()
    vis = out["visibility_filter"]
    assert (~vis).any() and vis.any()
    assert not F.grad[~vis].any() and F.grad[vis].any()
    # dL/dF[g, k] = sum_p c: every channel's column is the Gaussian's total weight
    assert torch.equal(F.grad[:, 0], F.grad[:, 1]) and torch.equal(F.grad[:, 0], F.grad[:, 2])


# ---- 9. pose -----------------------------------------------------------------
def test_pose_gradient_through_features(pkg, cuda):
    f = G.load("zero_bg_random")
    gi = U.tensor(f["g_image"], cuda)
    d_view = []
    for route in ("image", "features"):
        cam = U.camera_of(f)
        cam._wv = torch.tensor(np.asarray(f["wv"], np.float32), requires_grad=True)
        m, _, logits = U.gaussians_of(pkg, cuda, f)
        feats = torch.sigmoid(logits) if route == "features" else None
        _, out = U.render(pkg, cuda, f, feats, model=m, camera=cam)
        (out[route] * gi).sum().backward()
        d_view.append(cam._wv.grad.double().numpy())
    scale = np.abs(d_view[0]).max()
    err = np.abs(d_view[1] - d_view[0]).max()
    print(f"  d_view: features route vs image route: {err / scale:.3g} of scale {scale:.3g}")
    assert scale > 0 and err <= 1e-4 * scale


# ---- 10. validation ----------------------------------------------------------
def test_bad_feature_arguments(pkg, cuda):
    f = G.load("kat_two_coaxial")
    N = pkg._native
    for bad, exc in ((torch.ones(2, device=cuda), ValueError),              # rank
                     (torch.ones(2, 3, 1, device=cuda), ValueError),
                     (torch.ones(3, 4, device=cuda), ValueError),           # rows
                     (torch.ones(2, 4), RuntimeError),                      # device
                     (torch.ones(2, 4, dtype=torch.int32, device=cuda), TypeError),
                     (torch.ones(2, 0, device=cuda), ValueError),           # C outside 1..max
                     (torch.ones(2, N.GS_MAX_FEATURE_CHANNELS + 1, device=cuda), ValueError)):
        with pytest.raises(exc):
            U.render(pkg, cuda, f, bad)
    _, out = U.render(pkg, cuda, f, torch.ones(2, 2, dtype=torch.float64, device=cuda))  # cast on the tape
    assert out["features"].dtype == torch.float32 and out["features"].shape == (2, 64, 64)
    _, out = U.render(pkg, cuda, f, torch.ones(2, N.GS_MAX_FEATURE_CHANNELS, device=cuda))
    assert torch.equal(out["features"][-1], out["features"][0])
