"""Helpers of tests/test_distortion_cpu.py and tests/test_distortion_gpu.py:
the fp64 reference of the depth distortion and the fp32-sequential median
rule, both built from the weight image Wt[g, p] = c_g(p) that a render with
features = eye(N) returns (pinned to the oracle at 1e-4 by the feature
tests and, per float against an fp64 statement that owes nothing to the
replay kernels, by tests/test_replay_stage.py, which also checks k_dist_fwd
and k_dist_bwd themselves per pixel and per gradient partial); the same
formula in torch fp64 for the gradient reference; the built scene of
the cancellation test; and the child process of the cell-batch / no-bitmap
tests (the budgets are read at import)."""
import os
import sys

import numpy as np
import torch

import golden_io as G
from features_util import camera_depths, camera_of, gaussians_of, leaf_grad, np_, settings_of, tensor

U24 = 2.0 ** -24
NEAR_FAR = (0.1, 1000.0)


# ---- the formulas (numpy fp64 unless said otherwise) --------------------------
def mapped(z, near_far=None):
    """The mapped depth m(z): z, or 2DGS's NDC depth far (z - near) / ((far - near) z)."""
    if near_far is None:
        return z
    near, far = near_far
    return far * (z - near) / ((far - near) * z)


def prefix_distortion(c, m, xp=np):
    """2 sum_i c_i (m_i A_{i-1} - S_{i-1}) per column: c [n, P] weights in
    list order, m [n] (or [n, P]) ascending mapped depths."""
    if m.ndim == 1:
        m = m[:, None]
    cm = c * m
    A = xp.cumsum(c, 0)
    S = xp.cumsum(cm, 0)
    return 2.0 * (c * (m * (A - c) - (S - cm))).sum(0)


def brute_distortion(c, m):
    """sum_i sum_j c_i c_j |m_i - m_j| per column."""
    d = np.abs(m[:, None] - m[None, :])
    return np.einsum("ip,jp,ij->p", c, c, d)


def dD_dc(c, m):
    """2 [m_i (A_{i-1} + A_i - A_n) + S_n - S_i - S_{i-1}], [n, P]."""
    mm = m[:, None]
    A, S = np.cumsum(c, 0), np.cumsum(c * mm, 0)
    return 2.0 * (mm * ((A - c) + A - A[-1]) + S[-1] - S - (S - c * mm))


def dD_dm(c, m):
    """2 c_i (A_{i-1} + A_i - A_n), [n, P]."""
    A = np.cumsum(c, 0)
    return 2.0 * c * ((A - c) + A - A[-1])


def unshifted_fp32(c, m):
    """The prefix formula evaluated in fp32 on unshifted depths."""
    c, m = c.astype(np.float32), m.astype(np.float32)[:, None]
    cm = c * m
    A = np.cumsum(c, 0, dtype=np.float32)
    S = np.cumsum(cm, 0, dtype=np.float32)
    return np.float32(2.0) * (c * (m * (A - c) - (S - cm))).sum(0, dtype=np.float32)


def median_rule(c32):
    """Per column of c32 [n, P] (fp32, list order): the row of the first entry
    with c > 0 after whose addition the fp32 running sum is >= 0.5, else of the
    last entry with c > 0, else -1; and the final running sum."""
    n, P = c32.shape
    A = np.cumsum(c32, 0, dtype=np.float32) if n else np.zeros((0, P), np.float32)  # (sequential fp32 additions)
    pos = c32 > 0
    hit = pos & (A >= np.float32(0.5))
    first = np.where(hit.any(0), hit.argmax(0), -1) if n else np.full(P, -1)
    last = np.where(pos.any(0), n - 1 - pos[::-1].argmax(0), -1) if n else np.full(P, -1)
    return np.where(first >= 0, first, last), (A[-1] if n else np.zeros(P, np.float32))


def list_order(z32, vis):
    """The visible Gaussians in list order: by (bits of z, index)."""
    idx = np.nonzero(vis)[0]
    bits = z32[idx].view(np.uint32)
    return idx[np.lexsort((idx, bits))]


def bound(n_p, R_p):
    """8 (n_p + 1) 2^-24 R_p: twice the worst case of the fp32 chain (A and S
    carry n_p roundings each, on values <= 1 and <= R_p; every term adds one
    fma on a value <= R_p; the weights sum to at most 1; the leading factor 2)."""
    return 8.0 * (n_p + 1) * U24 * R_p


# ---- renders ------------------------------------------------------------------
def _settings(pkg, f, screen_filter=0.0):
    st = settings_of(pkg, f)
    st.screen_filter = screen_filter
    return st


def render(pkg, dev, f, model=None, camera=None, screen_filter=0.0, **kw):
    model = gaussians_of(pkg, dev, f)[0] if model is None else model
    out = pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(camera or camera_of(f), model,
                                                               _settings(pkg, f, screen_filter), **kw)
    return model, out


_REFERENCES: dict = {}


def reference(pkg, dev, f, key=None, near_far=None, screen_filter=0.0):
    """The fp64 reference of fixture f's maps (computed once per `key` and
    mapping, shared and left unchanged): one no-grad render with features =
    eye(N) gives Wt; z are the fp32 camera depths; per pixel D, n_p, R_p, the
    median Gaussian by the fp32-sequential rule and its running sum."""
    ck = (key, near_far, screen_filter)
    if key is not None and ck in _REFERENCES:
        return _REFERENCES[ck]
    n = f["xyz"].shape[0]
    H, W = int(f["height"]), int(f["width"])
    with torch.no_grad():
        _, out = render(pkg, dev, f, screen_filter=screen_filter, features=torch.eye(n, device=dev))
    Wt = out["features"].cpu().numpy().reshape(n, H * W)
    vis = out["visibility_filter"].cpu().numpy().astype(bool)
    z32 = camera_depths(f).astype(np.float32)
    order = list_order(z32, vis)
    c32 = Wt[order]
    c = c32.astype(np.float64)
    m = mapped(z32[order].astype(np.float64), near_far)
    D = prefix_distortion(c, m) if len(order) else np.zeros(H * W)
    on = c32 > 0
    n_p = on.sum(0)
    mm = np.broadcast_to(m[:, None], c.shape) if len(order) else np.zeros((0, H * W))
    R_p = (np.where(on, mm, -np.inf).max(0, initial=-np.inf) - np.where(on, mm, np.inf).min(0, initial=np.inf))
    R_p = np.where(n_p > 0, R_p, 0.0)
    row, A32 = median_rule(c32)
    med = np.where(row >= 0, order[np.maximum(row, 0)] if len(order) else -1, -1).astype(np.int32)
    res = dict(Wt=Wt, vis=vis, z=z32, order=order, c=c, m=m, D=D, n_p=n_p, R_p=R_p, median=med, A32=A32,
               alpha=out["alpha"].cpu().numpy().reshape(H * W), H=H, W=W)
    if key is not None:
        _REFERENCES[ck] = res
    return res


def maps(pkg, dev, f, near_far=None, screen_filter=0.0):
    """The maps under test, as numpy [H*W], with the forward's moments."""
    m, leaves, _ = gaussians_of(pkg, dev, f)
    _, out = render(pkg, dev, f, model=m, screen_filter=screen_filter, depth_distortion=True,
                    distortion_near_far=near_far)
    H, W = int(f["height"]), int(f["width"])
    for k, dt in (("distortion", torch.float32), ("median_depth", torch.float32), ("median_gaussian", torch.int32)):
        assert out[k].dtype == dt and tuple(out[k].shape) == (H, W), k
    assert out["distortion"].requires_grad and not out["median_depth"].requires_grad
    moments = out["distortion"].grad_fn.frame.distortion.moments  # (the rasterizer's frame keeps the pass)
    return dict(D=out["distortion"].detach().cpu().numpy().reshape(-1),
                median_depth=out["median_depth"].cpu().numpy().reshape(-1),
                median=out["median_gaussian"].cpu().numpy().reshape(-1),
                A=moments[0].cpu().numpy().reshape(-1), alpha=out["alpha"].detach().cpu().numpy().reshape(-1))


def check_forward(got, ref, what):
    err = np.abs(got["D"].astype(np.float64) - ref["D"])
    b = bound(ref["n_p"], ref["R_p"])
    worst = float((err / np.maximum(b, 1e-300))[ref["n_p"] >= 2].max()) if (ref["n_p"] >= 2).any() else 0.0
    print(f"  {what}: distortion max {ref['D'].max():.3g}, max err / bound = {worst:.3g}, "
          f"pixels with >= 2 contributors {(ref['n_p'] >= 2).sum()}")
    assert (err <= b).all(), f"{what}: distortion off by up to {worst:.3g} x its bound"


# ---- gradients ------------------------------------------------------------------
def cotangent(f, seed=11):
    H, W = int(f["height"]), int(f["width"])
    return np.random.default_rng(seed).uniform(-1, 1, (H, W)).astype(np.float32)


def view_depths(xyz, wv):
    """Camera-space z of xyz [N, 3] under the 4x4 view wv, in torch."""
    return xyz @ wv[2, :3] + wv[2, 3]


def reference_gradients(pkg, dev, f, g, near_far=None, screen_filter=0.0, pose=False, density_stats=None):
    """L_ref = sum_p g(p) D64(features[:, p], z_torch) through one
    differentiable render with features = eye(N); the leaves' gradients as
    numpy (and d_xi with pose=True).  density_stats: the reference's
    dL/dviewspace_points never surfaces as a .grad; its NDC norm is what the
    feature pass adds to these statistics (pinned by the density tests)."""
    n = f["xyz"].shape[0]
    model, leaves, _ = gaussians_of(pkg, dev, f)
    cam = pkg.CameraPose(camera_of(f)) if pose else camera_of(f)
    kw = {} if density_stats is None else {"density_stats": density_stats}
    _, out = render(pkg, dev, f, model=model, camera=cam, screen_filter=screen_filter,
                    features=torch.eye(n, device=dev), **kw)
    wv = cam.world_view_transform()
    z_t = view_depths(leaves["xyz"].double(), wv.to(dev).double())
    vis = out["visibility_filter"].cpu().numpy().astype(bool)
    order = torch.as_tensor(list_order(camera_depths(f).astype(np.float32), vis), device=dev)
    H, W = int(f["height"]), int(f["width"])
    c = out["features"].reshape(n, H * W)[order].double()
    D = prefix_distortion(c, mapped(z_t[order], near_far), xp=torch)
    (D * tensor(g, dev).reshape(-1).double()).sum().backward()
    res = {k: leaf_grad(k, t, n) for k, t in leaves.items()}
    if pose:
        res["xi"] = cam.xi.grad.double().numpy()
    return res


def gradients(pkg, dev, f, g, near_far=None, screen_filter=0.0, pose=False, density_stats=None):
    """L = sum_p g(p) distortion(p) of the render under test; the leaves' gradients."""
    n = f["xyz"].shape[0]
    model, leaves, _ = gaussians_of(pkg, dev, f)
    cam = pkg.CameraPose(camera_of(f)) if pose else camera_of(f)
    kw = {} if density_stats is None else {"density_stats": density_stats}
    _, out = render(pkg, dev, f, model=model, camera=cam, screen_filter=screen_filter, depth_distortion=True,
                    distortion_near_far=near_far, **kw)
    (out["distortion"] * tensor(g, dev)).sum().backward()
    res = {k: leaf_grad(k, t, n) for k, t in leaves.items()}
    res["D"] = np_(out["distortion"])
    res["median"] = out["median_gaussian"].cpu().numpy()
    if pose:
        res["xi"] = cam.xi.grad.double().numpy()
    return res


def check_gradients(got, ref, what):
    errs = []
    for k in ref:
        if k == "color_logits":
            assert not np.any(got[k]), f"{what}: d_color_logits from the distortion alone must be zero"
            continue
        rel = G.grad_rel_err(got[k], ref[k])
        print(f"  {what}: d_{k}: rel err {rel:.3g} of scale {np.abs(ref[k]).max():.3g}")
        assert np.abs(ref[k]).max() > 0, f"{what}: the reference's d_{k} is zero: nothing is compared"
        errs += G.check_grad(k, got[k], ref[k])
    assert not errs, (what, errs)


# ---- the built scene of the cancellation test -----------------------------------
def far_scene(tile=16):
    """64x64 px, 32 Gaussians at z in [2000, 2000.5], focal length 3200 px,
    lateral sigma 4..8 units (6..13 px): every pixel has several contributors
    whose depth spread is 2.5e-4 of their depth."""
    rng = np.random.default_rng(2000)
    n, W = 32, 64
    xyz = np.stack([rng.uniform(-14, 14, n), rng.uniform(-14, 14, n), rng.uniform(2000.0, 2000.5, n)], 1)
    sig = rng.uniform(4.0, 8.0, n)
    cov = np.stack([np.diag([s * s, s * s, 1e-4]) for s in sig])
    fov = 2.0 * np.arctan(0.5 * W / 3200.0)
    return dict(xyz=xyz.astype(np.float32), cov3d=cov.astype(np.float32),
                opacity=rng.uniform(0.15, 0.6, n).astype(np.float32),
                color_logits=rng.uniform(-1, 1, (n, 3)).astype(np.float32), width=W, height=W, cam_width=W,
                cam_height=W, fovx=fov, fovy=fov, wv=np.eye(4, dtype=np.float32), bg=np.zeros(3, np.float32),
                tile=tile)


# ---- the child process of the mode tests ----------------------------------------
KEYS = ("D", "median", "xyz", "cov3d", "opacity")


def mode_case(pkg, dev):
    f = G.load("tile32")
    return gradients(pkg, dev, f, cotangent(f))


def _child(mode, path):
    """tile32 under the budgets of this process's environment: the case twice
    (asserted bitwise equal by the parent), the batch size it ran with, saved."""
    import __graft_entry__ as ge
    pkg = ge.load_package()
    dev = torch.device("cuda:0")
    r1, r2 = (mode_case(pkg, dev) for _ in range(2))
    same = all(np.array_equal(r1[k], r2[k]) for k in KEYS)
    R = pkg.rasterizer
    T = int(R._T_SEEN[dev])
    batch = R.cell_batch(16, T)
    if mode == "batches":
        assert 1 <= batch < 16, batch
    else:
        assert R.live_bitmap_bytes(pkg._native.load(), 16, T, 1) == 0, "the bitmap is over its budget"
    np.savez(path, same=same, batch=batch, T=T, **{k: r1[k] for k in KEYS})


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    _child(sys.argv[1], sys.argv[2])
