"""Camera-pose gradients on the GPU: a world_view_transform that requires
grad receives dL/d(view) (gs_project_backward_pose), checked

  * against the reference's own fp64 view gradient on the pose fixtures
    (tests/golden/pose/, made by make_pose_golden.py), through both host paths;
  * against an identity in the per-Gaussian gradients of the same call
    (workgroup edges, the two-level reduction);
  * against a composed torch run for the SH view-direction term;
  * for bitwise reproducibility, view placement (device, dtype, shape), the
    data-parallel row callback, GraphedStep's refusal, and an end-to-end pose
    refinement with pose.CameraPose.

The bar is golden_io's gradient bar, per block of the 3x4 gradient:
|d - ref| <= 1e-4 * max|ref block| + 1e-7 for the R block and the t column."""
import functools
import math
import os

import numpy as np
import pytest
import torch

import golden_io as G
from sh_reference import sh_logits
from stubs import Cam

pytestmark = pytest.mark.gpu

POSE_GOLDEN = os.path.join(G.GOLDEN, "pose")
POSE_CASES = sorted(os.path.splitext(f)[0] for f in os.listdir(POSE_GOLDEN) if f.endswith(".npz"))
OUT_KEYS = ("image", "alpha", "depth", "viewspace_points", "conics", "radii", "visibility_filter")


def _load(name):
    z = np.load(os.path.join(POSE_GOLDEN, name + ".npz"))
    return {k: z[k] for k in z.files}


def view_errors(d_view, ref, what=""):
    """Failure strings for a [3+,4] gradient against `ref` at the bar, the R
    block and the t column each at its own scale; the figures are printed."""
    d = np.asarray(torch.as_tensor(d_view).detach().cpu().numpy(), np.float64)
    ref = np.asarray(torch.as_tensor(ref).detach().cpu().numpy(), np.float64)
    errs = []
    for blk, sl in (("R", np.s_[:3, :3]), ("t", np.s_[:3, 3])):
        scale = float(np.abs(ref[sl]).max())
        e = float(np.abs(d[sl] - ref[sl]).max())
        print(f"  {what} d_view {blk}: max err {e / max(scale, 1e-30):.3g} of scale {scale:.3g}")
        if not e <= G.GRAD_RTOL * scale + G.GRAD_ATOL:
            errs.append(f"{what} d_view {blk}: max abs err {e:.3g} > {G.GRAD_RTOL * scale + G.GRAD_ATOL:.3g}")
    return errs


class Stub:
    """A Gaussian object of tensors (get_xyz / get_covariance / get_features /
    get_opacity), each a leaf that requires grad unless given as a tensor."""

    def __init__(self, xyz, cov3d, feats, opacity, dev):
        leaf = lambda a: (a if isinstance(a, torch.Tensor) else
                          torch.tensor(np.asarray(a, np.float32), device=dev, requires_grad=True))
        self.xyz, self.cov, self.feats, self.op = leaf(xyz), leaf(cov3d), leaf(feats), leaf(opacity)

    get_xyz = property(lambda s: s.xyz)
    get_covariance = property(lambda s: s.cov)
    get_features = property(lambda s: s.feats)
    get_opacity = property(lambda s: s.op)

    def leaves(self):
        return [t for t in (self.xyz, self.cov, self.feats, self.op) if t.is_leaf]


def _feats(logits):
    n = len(logits)
    f = np.zeros((n, 16, 3), np.float32)
    f[:, 0, :] = np.asarray(logits, np.float32).reshape(n, 3)
    return f


def _fixture_gaussians(pkg, dev, f):
    n = f["xyz"].shape[0]
    if "scaling" in f:  # this package's model: the raw scaling / rotation path
        T = lambda a, shape=None: torch.tensor(np.asarray(a, np.float32)).reshape(shape or np.shape(a)).to(dev)
        m = pkg.GaussianModel()
        m._set(T(f["xyz"]), T(f["color_logits"], (n, 1, 3)), torch.zeros(n, 15, 3, device=dev), T(f["scaling"]),
               T(f["rotation"]), T(f["opacity_raw"], (n, 1)))
        return m, [m._xyz, m._scaling, m._rotation, m._features_dc, m._opacity]
    g = Stub(f["xyz"], f["cov3d"].reshape(n, 3, 3), _feats(f["color_logits"]), f["opacity"].reshape(n, 1), dev)
    return g, g.leaves()


def _loss(out, f, dev):
    t = lambda k: torch.tensor(np.asarray(f[k], np.float32), device=dev)
    L = (out["image"] * t("g_image")).sum() + (out["alpha"] * t("g_alpha")).sum() + (out["depth"] * t("g_depth")).sum()
    if "g_means2d" in f:
        L = L + (out["viewspace_points"] * t("g_means2d")).sum() + (out["conics"] * t("g_conics")).sum()
    return L


def _render_fixture(pkg, dev, f, view):
    g, leaves = _fixture_gaussians(pkg, dev, f)
    cam = Cam(f["cam_width"], f["cam_height"], f["fovx"], f["fovy"])
    cam._wv = view
    st = pkg.RenderSettings(image_height=int(f["height"]), image_width=int(f["width"]),
                            bg_color=torch.tensor(np.asarray(f["bg"], np.float32)))
    out = pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(cam, g, st)
    _loss(out, f, dev).backward()
    grads = [torch.zeros_like(t) if t.grad is None else t.grad.clone() for t in leaves]
    return [out[k].detach().clone() for k in OUT_KEYS], grads


@pytest.mark.parametrize("frame_calls", [True, False], ids=["frame", "stages"])
@pytest.mark.parametrize("name", POSE_CASES)
def test_pose_fixture(pkg, cuda, name, frame_calls):
    """d_view against the reference's fp64 view gradient; the per-Gaussian
    gradients and every forward output bitwise those of a call whose view does
    not require grad; the per-Gaussian gradients against the reference's."""
    RZ = pkg.rasterizer
    f = _load(name)
    saved = RZ._FRAME_CALLS
    try:
        RZ._FRAME_CALLS = frame_calls
        view = torch.tensor(f["wv"], requires_grad=True)
        outs, grads = _render_fixture(pkg, cuda, f, view)
        plain_outs, plain_grads = _render_fixture(pkg, cuda, f, torch.tensor(f["wv"]))
    finally:
        RZ._FRAME_CALLS = saved
    assert view.grad is not None, "the view received no gradient"
    assert view.grad.shape == (4, 4) and view.grad.dtype == torch.float32 and view.grad.device.type == "cpu"
    assert torch.count_nonzero(view.grad[3]) == 0
    errs = view_errors(view.grad, f["d_wv_f64"], name)
    for k, a, b in zip(OUT_KEYS, outs, plain_outs):
        assert torch.equal(a, b), k
    for a, b in zip(grads, plain_grads):
        assert torch.equal(a, b)
    n = f["xyz"].shape[0]
    if "scaling" in f:
        ref = [f["d_xyz"], f["d_scaling"], f["d_rotation"], f["d_color_logits"].reshape(n, 1, 3),
               f["d_opacity_raw"].reshape(n, 1)]
        got = grads
    else:
        ref = [f["d_xyz"], f["d_cov3d"], f["d_color_logits"], f["d_opacity"].reshape(n, 1)]
        got = [grads[0], grads[1], grads[2][:, 0], grads[3]]
    for i, (a, b) in enumerate(zip(got, ref)):
        errs += G.check_grad(f"{name}[{i}]", a.cpu().numpy(), b)
    if name == "pose_all_behind":
        assert torch.count_nonzero(view.grad) == 0 and int(outs[6].sum()) == 0
    assert not errs, errs


# ---- scenes made here (cov3d path, identity check) -------------------------

def _posed_view(dtype=torch.float32):
    a, b = 0.3, -0.2
    Ry = torch.tensor([[math.cos(a), 0, math.sin(a)], [0, 1, 0], [-math.sin(a), 0, math.cos(a)]], dtype=torch.float64)
    Rx = torch.tensor([[1, 0, 0], [0, math.cos(b), -math.sin(b)], [0, math.sin(b), math.cos(b)]], dtype=torch.float64)
    wv = torch.eye(4, dtype=torch.float64)
    wv[:3, :3] = Rx @ Ry
    wv[:3, 3] = torch.tensor([0.3, -0.2, 0.5], dtype=torch.float64)
    return wv.to(dtype)


@functools.lru_cache(maxsize=None)
def _scene(pkg, n, W, H, seed, sig=(0.02, 0.08)):
    """n Gaussians in front of _posed_view()'s camera, as CPU tensors: world
    xyz, cov3d = Rq diag(s^2) Rq^T, colour logits, opacity, random cotangents."""
    sc = pkg.synthetic.make_scene(n, W, H, seed=seed, sigma_range=sig)
    wv = _posed_view(torch.float64)
    xyz = ((sc.xyz.double() - wv[:3, 3]) @ wv[:3, :3]).float()
    Rq = pkg.build_rotation_matrix(sc.rotation)
    cov = (Rq * torch.exp(sc.scaling)[:, None, :] ** 2) @ Rq.transpose(1, 2)
    cov = 0.5 * (cov + cov.transpose(1, 2))
    g = torch.Generator().manual_seed(seed + 100)
    cot = [torch.rand(s, generator=g) * 2 - 1 for s in ((3, H, W), (1, H, W), (1, H, W))]
    return sc, xyz, cov, sc.features_dc[:, 0, :], torch.sigmoid(sc.opacity), cot


def _render_scene(pkg, dev, n, W, H, seed, view, sig=(0.02, 0.08)):
    sc, xyz, cov, logits, op, cot = _scene(pkg, n, W, H, seed, sig)
    g = Stub(xyz.numpy(), cov.numpy(), _feats(logits.numpy()), op.numpy(), dev)
    cam = Cam(W, H, sc.fovx, sc.fovy)
    cam._wv = view
    out = pkg.GaussianRenderer().render(cam, g, pkg.RenderSettings(H, W, torch.tensor([0.1, 0.2, 0.3])))
    (sum((out[k] * c.to(dev)).sum() for k, c in zip(("image", "alpha", "depth"), cot))).backward()
    return g, out


def _identity(view, g):
    """d_view [3,4] in fp64 from the per-Gaussian gradients of the same call
    (cov3d path, sh_degree 0, orthonormal R):
      d_t = R sum_g d_xyz[g],
      d_R = sum_g (R d_xyz[g]) Xw[g]^T + R (dS_g + dS_g^T) S_g."""
    R = view.detach()[:3, :3].double().cpu()
    X, S = g.xyz.detach().double().cpu(), g.cov.detach().double().cpu()
    dx, dS = g.xyz.grad.double().cpu(), g.cov.grad.double().cpu()
    d_t = R @ dx.sum(0)
    d_R = (dx @ R.T).T @ X + R @ ((dS + dS.transpose(1, 2)) @ S).sum(0)
    return torch.cat([d_R, d_t[:, None]], 1)


@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_workgroup_edges(pkg, cuda, n):
    """One Gaussian, one below / exactly / one above a workgroup of 256, and
    four workgroups with a part-filled last one, on a 32x32 image: the
    reduction against the identity in the same call's per-Gaussian gradients."""
    view = _posed_view().requires_grad_(True)
    g, out = _render_scene(pkg, cuda, n, 32, 32, 31, view)
    assert int(out["visibility_filter"].sum()) == n
    ref = _identity(view, g)
    assert ref.abs().max() > 0
    assert torch.count_nonzero(view.grad[3]) == 0
    errs = view_errors(view.grad, ref, f"N={n}")
    assert not errs, errs


def test_two_level_reduction(pkg, cuda):
    """70,000 Gaussians on 64x64: 274 partial rows, more than k_pose_reduce's
    256 threads, so some threads sum two rows before the tree.  Against the
    identity at the same bar.  The identity sums fp32-rounded gradients.
    Measured on an MI355X: R block 2.2e-08 of its scale (1.64e+04), t column
    4.6e-08 of its scale (6.42e+03) (printed below on every run)."""
    n = 70000
    view = _posed_view().requires_grad_(True)
    g, out = _render_scene(pkg, cuda, n, 64, 64, 32, view, sig=(0.002, 0.01))
    assert (n + 255) // 256 > 256 and int(out["visibility_filter"].sum()) > 60000
    errs = view_errors(view.grad, _identity(view, g), f"N={n}")
    assert not errs, errs


@pytest.mark.parametrize("n,W,sig", [(1000, 32, (0.02, 0.08)), (70000, 64, (0.002, 0.01))])
def test_reproducible(pkg, cuda, n, W, sig):
    got = []
    for _ in range(2):
        view = _posed_view().requires_grad_(True)
        g, out = _render_scene(pkg, cuda, n, W, W, 33, view, sig=sig)
        got.append([view.grad.clone(), g.xyz.grad.clone(), g.cov.grad.clone(), out["image"].detach().clone()])
    assert got[0][0].abs().max() > 0
    for a, b in zip(*got):
        assert torch.equal(a, b)


def test_view_placement(pkg, cuda):
    """The gradient returns to the view's own device, dtype and shape."""
    ref = None
    for make in (lambda: _posed_view(), lambda: _posed_view(torch.float64), lambda: _posed_view().to(cuda)):
        view = make().requires_grad_(True)
        _render_scene(pkg, cuda, 300, 32, 32, 34, view)
        assert view.grad.shape == (4, 4) and view.grad.dtype == view.dtype and view.grad.device == view.device
        assert torch.count_nonzero(view.grad[3]) == 0
        if ref is None:
            ref = view.grad.clone()
        assert torch.equal(view.grad.float().cpu(), ref)  # (the same fp32 sum, cast)
    # a [3,4] view straight into rasterize(): a [3,4] gradient; and a non-leaf view (here 2 x leaf)
    sc, xyz, cov, logits, op, cot = _scene(pkg, 300, 32, 32, 34)
    st = pkg.RenderSettings(32, 32, torch.tensor([0.1, 0.2, 0.3]))
    cam = Cam(32, 32, sc.fovx, sc.fovy, _posed_view().numpy())
    leaf = (0.5 * _posed_view()[:3]).to(cuda).requires_grad_(True)
    o = pkg.rasterize(pkg.camera_params(cam, st), xyz.to(cuda), cov.to(cuda), None, None, logits.to(cuda),
                      op[:, 0].to(cuda), view=2.0 * leaf)
    sum((t * c.to(cuda)).sum() for t, c in zip(o[:3], cot)).backward()
    assert leaf.grad.shape == (3, 4) and torch.equal(leaf.grad.cpu(), 2.0 * ref[:3])
    with pytest.raises(ValueError, match=r"\[3,4\] or \[4,4\]"):
        pkg.rasterize(pkg.camera_params(cam, st), xyz.to(cuda), cov.to(cuda), None, None, logits.to(cuda),
                      op[:, 0].to(cuda), view=torch.zeros(12, requires_grad=True))


@pytest.mark.parametrize("frame_calls", [True, False], ids=["frame", "stages"])
def test_empty_model_zero_gradient(pkg, cuda, frame_calls):
    """N = 0: the reference's background early return; the view's gradient is
    all zeros (gs_project_backward_pose with nothing to sum), not None."""
    RZ = pkg.rasterizer
    saved = RZ._FRAME_CALLS
    try:
        RZ._FRAME_CALLS = frame_calls
        g = Stub(np.zeros((0, 3)), np.zeros((0, 3, 3)), np.zeros((0, 16, 3)), np.zeros((0, 1)), cuda)
        view = _posed_view().requires_grad_(True)
        cam = Cam(32, 32, 1.0, 1.0)
        cam._wv = view
        out = pkg.GaussianRenderer().render(cam, g, pkg.RenderSettings(32, 32, torch.tensor([0.2, 0.3, 0.4])))
        (out["image"].sum() + out["alpha"].sum()).backward()
    finally:
        RZ._FRAME_CALLS = saved
    assert view.grad is not None and view.grad.shape == (4, 4) and torch.count_nonzero(view.grad) == 0


@pytest.mark.parametrize("frame_calls", [True, False], ids=["frame", "stages"])
def test_row_callback_runs_once_over_every_row(pkg, cuda, frame_calls):
    """With the data-parallel reduction's row callback attached, a pose
    backward runs as one range and then reports rows [0, n), whatever the
    number of ranges asked for; gradients equal the plain backward's."""
    RZ = pkg.rasterizer
    n = 3000
    sc = pkg.synthetic.make_scene(n, 64, 64, seed=35, sigma_range=(0.01, 0.05))
    m = pkg.synthetic.to_model(sc, pkg.GaussianModel, cuda)
    cam = pkg.camera_params(Cam(64, 64, sc.fovx, sc.fovy), pkg.RenderSettings(64, 64, torch.zeros(3)))
    raw = (m._xyz.detach(), None, m._scaling.detach(), m._rotation.detach(), m._features_dc.detach()[:, 0, :],
           m._opacity.detach())
    saved = RZ._FRAME_CALLS
    got = []
    try:
        RZ._FRAME_CALLS = frame_calls
        for pose in (True, False):
            img, al, dp, m2, cn, rd, vi, fr = RZ.forward_pipeline(cam, *raw, opacity_is_logit=True, need_grad=True)
            assert fr.calls == frame_calls
            seen = []
            d_view = torch.full((12,), float("nan"), device=cuda) if pose else None
            d = RZ.backward_pipeline(cam, fr, *raw, m2, cn, torch.ones_like(img), None, None, None, None,
                                     opacity_is_logit=True, outputs=(img, al, dp), d_view=d_view,
                                     out={"_rows_ready": lambda lo, hi: seen.append((lo, hi)), "_chunks": 3})
            assert seen == ([(0, n)] if pose else [(n * k // 3, n * (k + 1) // 3) for k in range(3)])
            got.append([t.clone() for t in d if t is not None])
            if pose:
                assert torch.isfinite(d_view).all() and d_view.abs().max() > 0
    finally:
        RZ._FRAME_CALLS = saved
    for a, b in zip(*got):
        assert torch.equal(a, b)


@pytest.mark.parametrize("degree", [1, 3])
def test_sh_view_direction_term(pkg, cuda, degree):
    """sh_degree > 0: the colour depends on the pose through campos = -R^T t.
    Expectation: a composed run whose logits are the torch SH statement
    (sh_reference.sh_logits) with campos built from the same grad-requiring
    view, rendered at degree 0 through a stub Gaussian object."""
    n, W, H = 2000, 64, 48
    sc, xyz, cov, logits, op, cot = _scene(pkg, n, W, H, 36)
    g = torch.Generator().manual_seed(37)
    rest = 2.0 * torch.randn(n, 15, 3, generator=g)  # (strong view dependence: see the SH part below)
    dc = torch.rand(n, 3, generator=g) * 4 - 2
    st = lambda d: pkg.RenderSettings(H, W, torch.tensor([0.1, 0.2, 0.3]), sh_degree=d)
    loss = lambda out: sum((out[k] * c.to(cuda)).sum() for k, c in zip(("image", "alpha", "depth"), cot))

    view = _posed_view().to(cuda).requires_grad_(True)
    cam = Cam(W, H, sc.fovx, sc.fovy)
    cam._wv = view
    feats = torch.cat([dc[:, None, :], rest], 1).numpy()
    direct = Stub(xyz.numpy(), cov.numpy(), feats, op.numpy(), cuda)
    out = pkg.GaussianRenderer().render(cam, direct, st(degree))
    loss(out).backward()
    assert int(out["visibility_filter"].sum()) == n

    view2 = _posed_view().to(cuda).requires_grad_(True)
    cam2 = Cam(W, H, sc.fovx, sc.fovy)
    cam2._wv = view2
    campos = -(view2[:3, :3].T @ view2[:3, 3])
    lg = sh_logits(xyz.to(cuda), dc.to(cuda), rest.to(cuda), campos, degree)
    composed = Stub(xyz.numpy(), cov.numpy(), lg[:, None, :], op.numpy(), cuda)
    out2 = pkg.GaussianRenderer().render(cam2, composed, st(0))
    loss(out2).backward()

    assert (out["image"] - out2["image"]).abs().max().item() <= 1e-5
    # the SH term is a visible part of the expectation: above three times
    # the bar, so a d_view without it would fail below
    plain = _posed_view().to(cuda).requires_grad_(True)
    cam3 = Cam(W, H, sc.fovx, sc.fovy)
    cam3._wv = plain
    out3 = pkg.GaussianRenderer().render(cam3, Stub(xyz.numpy(), cov.numpy(), lg.detach()[:, None, :], op.numpy(), cuda),
                                         st(0))
    loss(out3).backward()
    sh_part = (view2.grad - plain.grad)[:3].abs().max().item()
    print(f"  degree {degree}: SH part of d_view up to {sh_part:.3g} (d_view up to {view2.grad.abs().max().item():.3g})")
    assert sh_part > 3 * (G.GRAD_RTOL * view2.grad.abs().max().item() + G.GRAD_ATOL)
    errs = view_errors(view.grad, view2.grad, f"sh_degree={degree}")
    assert not errs, errs


def test_graphed_step_refuses_a_view_that_requires_grad(pkg, cuda):
    sc = pkg.synthetic.make_scene(500, 64, 64, seed=38, sigma_range=(0.01, 0.05))
    m = pkg.synthetic.to_model(sc, pkg.GaussianModel, cuda)
    st = pkg.RenderSettings(64, 64, torch.zeros(3))
    cot = [torch.ones(3, 64, 64), torch.zeros(1, 64, 64), torch.zeros(1, 64, 64)]
    with pytest.raises(ValueError, match="requires grad"):
        pkg.GraphedStep(pkg.GaussianRenderer(), pkg.CameraPose(Cam(64, 64, sc.fovx, sc.fovy)), m, st, cot)


def test_pose_refinement(pkg, cuda):
    """CameraPose on a 64x64 scene of 500 Gaussians: from a pose about 2 degrees
    and 2 % of the scene depth off, Adam on the twist lowers both the image
    loss and the pose error (no factor fixed in advance; the achieved ratios
    are printed)."""
    n, W, H = 500, 64, 64
    sc = pkg.synthetic.make_scene(n, W, H, seed=39, sigma_range=(0.08, 0.25))
    m = pkg.synthetic.to_model(sc, pkg.GaussianModel, cuda)
    for p in m.parameters():
        p.requires_grad_(False)
    st = pkg.RenderSettings(H, W, torch.zeros(3))
    r = pkg.GaussianRenderer()
    true = _posed_view()
    true[:3, 3] = torch.tensor([0.1, -0.05, 0.3])
    with torch.no_grad():
        target = r.render(Cam(W, H, sc.fovx, sc.fovy, true.numpy()), m, st)["image"].clone()
    # perturbed start: 2 degrees about (1, -1, 0.5) / 1.5, 0.08 (2 % of depth 4) along (-1, 0.5, 1) / 1.5
    off = torch.cat([0.08 * torch.tensor([-1.0, 0.5, 1.0]) / 1.5, math.radians(2.0) * torch.tensor([1.0, -1.0, 0.5]) / 1.5])
    start = pkg.se3_exp(off) @ true
    pose = pkg.CameraPose(Cam(W, H, sc.fovx, sc.fovy, start.numpy()))
    opt = torch.optim.Adam(pose.parameters(), lr=2e-3)
    err = lambda: (pose.world_view_transform().detach() - true)[:3].norm().item()
    e0, losses = err(), []
    for it in range(200):
        opt.zero_grad()
        loss = ((r.render(pose, m, st)["image"] - target) ** 2).mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        final = ((r.render(pose, m, st)["image"] - target) ** 2).mean().item()
    e1 = err()
    print(f"  pose refinement: loss {losses[0]:.3g} -> {final:.3g} (x {final / losses[0]:.3g}), "
          f"pose error {e0:.3g} -> {e1:.3g} (x {e1 / e0:.3g})")
    assert pose.xi.grad is not None and torch.isfinite(pose.xi.grad).all()
    assert final < losses[0] and e1 < e0
