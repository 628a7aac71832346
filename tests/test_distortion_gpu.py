"""Depth distortion and median depth through the blend
(render(..., depth_distortion=True)): the forward against an fp64 reference
built from the weight image of a features = eye(N) render, the median exact,
the gradients against torch fp64 autograd of the same formula through the
feature backward, the other outputs bit for bit, the cell-batch and no-bitmap
modes, and one trainer step.

Forward bound per pixel: 8 (n_p + 1) 2^-24 R_p (distortion_util.bound), n_p the
pixel's contributors and R_p the spread of their mapped depths.  Gradients:
golden_io.check_grad's 1e-4 max|d_ref| + 1e-7 per tensor."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import distortion_util as DU
import features_util as FU
import golden_io as G

pytestmark = pytest.mark.gpu

FORWARD = ["zero_bg_random", "random_bg", "tile8", "tile12", "tile32", "radius80_tile8", "saturate", "offscreen",
           "posed_camera", "model_random"]
GRADS = ["zero_bg_random", "tile8", "tile32", "saturate", "posed_camera", "model_random"]
OUTPUTS = ("image", "alpha", "depth", "viewspace_points", "conics", "radii", "visibility_filter")


def _fixture(name):
    return DU.far_scene() if name == "far_scene" else G.load(name)


# ---- 1. closed form ------------------------------------------------------------
def test_two_coaxial_closed_form(pkg, cuda):
    f = G.load("kat_two_coaxial")
    ref = DU.reference(pkg, cuda, f, "kat_two_coaxial")
    got = DU.maps(pkg, cuda, f)
    z = ref["z"].astype(np.float64)
    i, j = ref["order"]
    want = 2.0 * ref["Wt"][i].astype(np.float64) * ref["Wt"][j].astype(np.float64) * (z[j] - z[i])
    assert z[j] > z[i] and want.max() > 0
    err = np.abs(got["D"] - want)
    assert (err <= DU.bound(ref["n_p"], ref["R_p"])).all(), float(err.max())


def test_single_gaussian_has_no_distortion(pkg, cuda):
    f = G.load("kat_single")
    got = DU.maps(pkg, cuda, f)
    assert not got["D"].any() and (got["median"] >= 0).any()


# ---- 2. forward against the fp64 reference ------------------------------------
@pytest.mark.parametrize("name", FORWARD)
def test_forward_matches_fp64_reference(pkg, cuda, name):
    f = G.load(name)
    ref = DU.reference(pkg, cuda, f, name)
    assert (ref["n_p"] >= 2).any(), "no pixel with two contributors: the wrong scene for this test"
    DU.check_forward(DU.maps(pkg, cuda, f), ref, name)


def test_shift_is_irrelevant_in_fp64(pkg, cuda):
    ref = DU.reference(pkg, cuda, G.load("zero_bg_random"), "zero_bg_random")
    shifted = DU.prefix_distortion(ref["c"], ref["m"] - ref["m"][0])
    assert np.abs(shifted - ref["D"]).max() <= 1e-12 * max(ref["D"].max(), 1e-30)


# ---- 3. cancellation -----------------------------------------------------------
def test_far_scene_survives_cancellation(pkg, cuda):
    f = DU.far_scene()
    ref = DU.reference(pkg, cuda, f, "far_scene")
    assert ref["z"].min() >= 2000.0 and ref["z"].max() <= 2000.5
    assert np.median(ref["n_p"]) >= 3, "several contributors per pixel"
    b = DU.bound(ref["n_p"], ref["R_p"])
    naive = DU.unshifted_fp32(ref["c"], ref["m"]).astype(np.float64)
    broken = np.abs(naive - ref["D"]) > b
    print(f"  far_scene: the unshifted fp32 formula breaks the bound on {broken.sum()} of {broken.size} pixels "
          f"(worst {float((np.abs(naive - ref['D']) / np.maximum(b, 1e-300))[ref['n_p'] >= 2].max()):.3g} x)")
    assert broken.any(), "an unshifted fp32 evaluation survives this scene: the wrong scene for this test"
    DU.check_forward(DU.maps(pkg, cuda, f), ref, "far_scene")


# ---- 4. inverse mapping ----------------------------------------------------------
@pytest.mark.parametrize("name", ["zero_bg_random", "far_scene"])
def test_inverse_mapping(pkg, cuda, name):
    f = _fixture(name)
    ref = DU.reference(pkg, cuda, f, name, near_far=DU.NEAR_FAR)
    assert (ref["n_p"] >= 2).any() and ref["R_p"].max() < 1.0
    DU.check_forward(DU.maps(pkg, cuda, f, near_far=DU.NEAR_FAR), ref, name + " (inverse)")


# ---- 5. median, exact ------------------------------------------------------------
@pytest.mark.parametrize("name", FORWARD)
def test_median_is_exact(pkg, cuda, name):
    f = G.load(name)
    ref = DU.reference(pkg, cuda, f, name)
    got = DU.maps(pkg, cuda, f)
    assert np.array_equal(got["median"], ref["median"])
    none = ~(ref["Wt"] > 0).any(0)
    assert np.array_equal(got["median"] == -1, none)
    want_z = np.where(none, np.float32(0), ref["z"][np.maximum(got["median"], 0)]).astype(np.float32)
    assert np.array_equal(got["median_depth"].view(np.uint32), want_z.view(np.uint32))  # (the record depths' bits)
    assert np.array_equal(got["A"].view(np.uint32), got["alpha"].view(np.uint32))
    assert np.array_equal(got["A"].view(np.uint32), ref["A32"].view(np.uint32))


def test_nothing_visible(pkg, cuda):
    f = G.load("all_behind")
    m, leaves, _ = FU.gaussians_of(pkg, cuda, f)
    _, out = DU.render(pkg, cuda, f, model=m, depth_distortion=True)
    assert out["distortion"].shape == (64, 64) and not out["distortion"].any()
    assert not out["median_depth"].any() and (out["median_gaussian"] == -1).all()
    assert out["median_gaussian"].dtype == torch.int32
    out["distortion"].sum().backward()
    for k, t in leaves.items():
        assert t.grad is None or not t.grad.any(), k


# ---- 6. gradients ------------------------------------------------------------------
@pytest.mark.parametrize("name", GRADS + ["far_scene"])
def test_gradients_match_fp64_autograd(pkg, cuda, name):
    f = _fixture(name)
    g = DU.cotangent(f)
    pose = name == "posed_camera"
    ref = DU.reference_gradients(pkg, cuda, f, g, pose=pose)
    got = DU.gradients(pkg, cuda, f, g, pose=pose)
    DU.check_gradients(got, ref, name)


@pytest.mark.parametrize("name", ["zero_bg_random", "far_scene"])
def test_gradients_inverse_mapping(pkg, cuda, name):
    f = _fixture(name)
    g = DU.cotangent(f)
    ref = DU.reference_gradients(pkg, cuda, f, g, near_far=DU.NEAR_FAR)
    got = DU.gradients(pkg, cuda, f, g, near_far=DU.NEAR_FAR)
    DU.check_gradients(got, ref, name + " (inverse)")


# ---- 7. nothing else moves -------------------------------------------------------------
def _colour_loss(out, f, dev):
    return sum((out[k] * FU.tensor(f["g_" + k], dev)).sum() for k in ("image", "alpha", "depth"))


@pytest.mark.parametrize("with_features", [False, True])
@pytest.mark.parametrize("name", ["model_random", "random_bg", "tile12"])
def test_colour_outputs_and_gradients_untouched(pkg, cuda, name, with_features):
    f = G.load(name)
    n = f["xyz"].shape[0]
    res = []
    for distortion in (False, True):
        m, leaves, _ = FU.gaussians_of(pkg, cuda, f)
        kw = {"depth_distortion": True} if distortion else {}
        if with_features:
            kw["features"] = torch.rand((n, 5), generator=torch.Generator().manual_seed(3)).to(cuda)
        _, out = DU.render(pkg, cuda, f, model=m, **kw)
        _colour_loss(out, f, cuda).backward()
        res.append((out, leaves))
    (a, la), (b, lb) = res
    assert "distortion" not in a and "median_depth" not in a and "distortion" in b
    for k in OUTPUTS + (("features",) if with_features else ()):
        assert a[k].dtype == b[k].dtype and torch.equal(a[k], b[k]), k
    for k in la:
        assert la[k].grad is not None and torch.equal(la[k].grad, lb[k].grad), k


def test_features_and_distortion_in_one_loss(pkg, cuda):
    f = G.load("tile12")
    n = f["xyz"].shape[0]
    g = DU.cotangent(f)
    gF = np.random.default_rng(5).uniform(-1, 1, (5, int(f["height"]), int(f["width"]))).astype(np.float32)
    F0 = torch.rand((n, 5), generator=torch.Generator().manual_seed(3))
    grads = []
    for use_f, use_d in ((True, False), (False, True), (True, True)):
        m, leaves, _ = FU.gaussians_of(pkg, cuda, f)
        F = F0.to(cuda).requires_grad_()
        _, out = DU.render(pkg, cuda, f, model=m, features=F, depth_distortion=True, dominant=True,
                           contribution_stats=pkg.ContributionStats(n, cuda))
        L = 0
        if use_f:
            L = L + (out["features"] * FU.tensor(gF, cuda)).sum()
        if use_d:
            L = L + (out["distortion"] * FU.tensor(g, cuda)).sum()
        L.backward()
        d = {k: FU.leaf_grad(k, t, n).astype(np.float64) for k, t in leaves.items()}
        d["features"] = np.zeros((n, 5)) if F.grad is None else FU.np_(F.grad).astype(np.float64)
        grads.append(d)
        assert out["dominant_gaussian"].shape == out["median_gaussian"].shape
    errs = []
    for k in grads[0]:
        errs += G.check_grad(k, grads[2][k], grads[0][k] + grads[1][k])
    assert not errs, errs
    assert not grads[1]["features"].any()


def test_sh_colour_composes(pkg, cuda):
    """SH colour (degree 2) alongside: the distortion reads no colour, so its
    map is the DC render's bit for bit, and its gradients within check_grad."""
    f = G.load("model_random")
    g = DU.cotangent(f)
    res = []
    for degree in (0, 2):
        m, leaves, _ = FU.gaussians_of(pkg, cuda, f)
        with torch.no_grad():
            m._features_rest.copy_(torch.rand(m._features_rest.shape, generator=torch.Generator().manual_seed(1)) - 0.5)
        st = FU.settings_of(pkg, f)
        st.sh_degree = degree
        out = pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(FU.camera_of(f), m, st, depth_distortion=True)
        (out["distortion"] * FU.tensor(g, cuda)).sum().backward()
        res.append((out["distortion"].detach().clone(), leaves["xyz"].grad.clone()))
    assert torch.equal(res[0][0], res[1][0])
    assert res[0][1].abs().max() > 0 and not G.check_grad("xyz", FU.np_(res[1][1]), FU.np_(res[0][1]))


# ---- 8. modes ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def one_batch(pkg, cuda):
    """tile32 in one batch, with the liveness bitmap: the case and its reference."""
    f = G.load("tile32")
    one, again = (DU.mode_case(pkg, cuda) for _ in range(2))
    for k in DU.KEYS:
        assert np.array_equal(one[k], again[k]), k
    T = int(pkg.rasterizer._T_SEEN[cuda])
    assert pkg.rasterizer.cell_batch(16, T) == 16
    return one, DU.reference_gradients(pkg, cuda, f, DU.cotangent(f)), T


@pytest.mark.parametrize("mode", ["batches", "no_bitmap"])
def test_modes_in_a_child_process(pkg, cuda, tmp_path, one_batch, mode):
    """GS_PARTIAL_BUDGET / GS_LIVE_BUDGET are read at import: a child process
    renders tile32's 16 cells in batches of 5, or without the liveness bitmap."""
    one, ref, T = one_batch
    path = str(tmp_path / (mode + ".npz"))
    env = dict(os.environ)
    if mode == "batches":
        env["GS_PARTIAL_BUDGET"] = str(41 * T * 5 + 1)  # 5 cells per batch: 5 + 5 + 5 + 1
    else:
        env["GS_LIVE_BUDGET"] = "1"
    subprocess.run([sys.executable, os.path.join(G.ROOT, "tests", "distortion_util.py"), mode, path], check=True,
                   env=env, timeout=300)
    b = np.load(path)
    assert bool(b["same"]) and int(b["T"]) == T
    assert int(b["batch"]) == (5 if mode == "batches" else 16)
    assert np.array_equal(b["D"], one["D"]) and np.array_equal(b["median"], one["median"])
    DU.check_gradients({k: b[k] for k in ("xyz", "cov3d", "opacity")},
                       {k: ref[k] for k in ("xyz", "cov3d", "opacity")}, "tile32 " + mode)


def test_screen_filter(pkg, cuda):
    f = G.load("zero_bg_random")
    ref = DU.reference(pkg, cuda, f, "zero_bg_random", screen_filter=0.3)
    plain = DU.reference(pkg, cuda, f, "zero_bg_random")
    assert not np.array_equal(ref["Wt"], plain["Wt"]), "the filter changes the weights"
    DU.check_forward(DU.maps(pkg, cuda, f, screen_filter=0.3), ref, "zero_bg_random (filter 0.3)")
    g = DU.cotangent(f)
    DU.check_gradients(DU.gradients(pkg, cuda, f, g, screen_filter=0.3),
                       DU.reference_gradients(pkg, cuda, f, g, screen_filter=0.3), "zero_bg_random (filter 0.3)")


def test_density_statistics_see_the_distortion(pkg, cuda):
    f = G.load("zero_bg_random")
    n = f["xyz"].shape[0]
    g = DU.cotangent(f)
    want, got = pkg.DensityStats(n, cuda), pkg.DensityStats(n, cuda)
    DU.reference_gradients(pkg, cuda, f, g, density_stats=want)
    DU.gradients(pkg, cuda, f, g, density_stats=got)
    assert torch.equal(want.denom, got.denom) and torch.equal(want.max_radii, got.max_radii)
    w = FU.np_(want.grad_accum)
    errs = G.check_grad("stats", FU.np_(got.grad_accum), w)
    assert w.max() > 0 and not errs, errs


# ---- 9. trainer ------------------------------------------------------------------------------
def _count_calls(monkeypatch, lib):
    calls = {"gs_blend_distortion_forward": 0, "gs_blend_distortion_backward": 0}
    for name in calls:
        fn = getattr(lib, name)

        def wrapper(*a, _fn=fn, _name=name):
            calls[_name] += 1
            return _fn(*a)
        monkeypatch.setattr(lib, name, wrapper)
    return calls


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-30))


def test_trainer_step_matches_a_step_composed_by_hand(pkg, cuda, tmp_path, monkeypatch):
    from scene_util import load_scene, write_scene_files
    from test_trainer_parity_gpu import NAMES, _adam, lr_at
    size, lam = 48, 0.5
    write_scene_files(tmp_path, n_views=4, size=size)
    ds = load_scene(pkg, tmp_path, cuda, size, split=False)
    kw = dict(iterations=3, densify_from_iter=10 ** 6, densify_until_iter=10 ** 6, num_random_points=2000,
              log_interval=1, output_path=str(tmp_path / "out"), position_lr_init=1.6e-3, position_lr_final=1.6e-5)
    calls = _count_calls(monkeypatch, pkg._native.load())

    # lambda_distortion = 0: the launches of today (neither entry point is called)
    tr0 = pkg.GaussianTrainer(pkg.TrainingConfig(**kw), ds)
    tr0.setup()
    tr0.train(1)
    assert calls == {"gs_blend_distortion_forward": 0, "gs_blend_distortion_backward": 0}

    cfg = pkg.TrainingConfig(lambda_distortion=lam, distortion_from_iter=1, **kw)
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    with torch.no_grad():  # (anisotropic, as tests/test_trainer_parity_gpu.py: well-conditioned rotation gradients)
        gen = torch.Generator().manual_seed(5)
        tr.gaussians._scaling.add_(torch.empty(tr.gaussians._scaling.shape).uniform_(-0.7, 0.7, generator=gen).to(cuda))
    init = [q.detach().clone() for q in tr.gaussians.parameter_list()]
    cam = ds.get_train_cameras()[int(tr._perm[1 % len(ds.get_train_cameras())])]

    # by hand: render, photometric_loss + lam * distortion.mean(), torch Adam
    m = pkg.GaussianModel()
    m._set(*[t.clone() for t in init])
    p = m.parameter_list()
    opt = _adam(cfg, p)
    out = pkg.GaussianRenderer().render(cam, m, pkg.RenderSettings(size, size, torch.zeros(3)), depth_distortion=True)
    mean_d = float(out["distortion"].detach().mean())
    (pkg.photometric_loss(out["image"], cam._image, cfg.lambda_dssim)[0] + lam * out["distortion"].mean()).backward()
    base = lr_at(cfg, 1)
    for grp, lr in zip(opt.param_groups, (cfg.position_lr_init, cfg.feature_lr, cfg.opacity_lr, cfg.scaling_lr,
                                           cfg.rotation_lr)):
        grp["lr"] = base * (lr / cfg.position_lr_init)
    opt.step()
    assert mean_d > 0, "the scene has no distortion: nothing is compared"
    before = dict(calls)

    tr.train(1)
    assert calls["gs_blend_distortion_forward"] == before["gs_blend_distortion_forward"] + 1
    assert calls["gs_blend_distortion_backward"] >= before["gs_blend_distortion_backward"] + 1
    got = tr.gaussians.parameter_list()
    for name, a, b, i0 in zip(NAMES, got, p, init):
        e = _rel(a, b)
        print(f"  {name:14s} param rel err {e:.2e} (moved {_rel(b, i0):.2e})")
        assert e <= 1e-5, (name, e)
    fused = tr.optimizer.optimizer
    for name, a, b in zip(NAMES, got, p):
        st_g, st_r = fused.state.get(a, {}), opt.state.get(b, {})
        assert bool(st_g) == bool(st_r), name
        if st_r:
            em, ev = _rel(st_g["exp_avg"], st_r["exp_avg"]), _rel(st_g["exp_avg_sq"], st_r["exp_avg_sq"])
            print(f"  {name:14s} m rel err {em:.2e}  v rel err {ev:.2e}")
            assert em <= 1e-4 and ev <= 1e-4, (name, em, ev)
    # the term changes the step: without it the first moment of xyz differs
    plain = pkg.GaussianModel()
    plain._set(*[t.clone() for t in init])
    o2 = pkg.GaussianRenderer().render(cam, plain, pkg.RenderSettings(size, size, torch.zeros(3)))
    pkg.photometric_loss(o2["image"], cam._image, cfg.lambda_dssim)[0].backward()
    assert _rel(plain._xyz.grad, p[0].grad) > 1e-3
