"""Density-control statistics on the device: gs_density_accumulate against an
fp64 numpy statement, the renderer's accumulation end to end against the
pinned oracle's dL/dmeans2d, and the densification that reads the statistics
against the fp64 torch statement of tests/test_densify.py."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

import features_util as FU
import golden_io as G
from test_densify import LARGE, NAMES, SMALL, _make_safe, _model, ref_densify

pytestmark = pytest.mark.gpu


def _np(t):
    return t.detach().cpu().numpy()


# ---- the kernel ---------------------------------------------------------------
KW, KH, KN = 52, 44, 300  # W != H: the two scale factors cannot be swapped; two 256-blocks, the second partial


def _kernel_inputs():
    rng = np.random.default_rng(5)
    return dict(sums=rng.normal(0, 1e-3, (KN, 10)).astype(np.float32),
                gm=rng.normal(0, 1e-3, (KN, 2)).astype(np.float32),
                radii=rng.uniform(0.5, 40.0, KN).astype(np.float32),
                vis=rng.random(KN) > 1 / 3,
                start=[rng.uniform(0.0, 0.05, KN).astype(np.float32),          # grad_accum
                       rng.integers(0, 9, KN).astype(np.float32),              # denom
                       rng.uniform(0.0, 30.0, KN).astype(np.float32)])         # max_radii


def _statement(acc, den, rad, vis, sums, gm, radii, W, H):
    """The header's statement in fp64, on the fp32 values the kernel reads."""
    gx = (0.0 if sums is None else sums[:, 0].astype(np.float64)) + (0.0 if gm is None else gm[:, 0].astype(np.float64))
    gy = (0.0 if sums is None else sums[:, 1].astype(np.float64)) + (0.0 if gm is None else gm[:, 1].astype(np.float64))
    norm = np.sqrt((0.5 * W * gx) ** 2 + (0.5 * H * gy) ** 2) * np.ones(len(vis))
    return (np.where(vis, acc + norm, acc), np.where(vis, den + 1.0, den),
            np.where(vis, np.maximum(rad, radii.astype(np.float64)), rad))


@pytest.mark.parametrize("variant", ["both", "no_grad_sums", "no_g_means2d", "neither"])
def test_kernel_matches_fp64_statement(pkg, cuda, variant):
    N = pkg._native
    lib = N.load()
    k = _kernel_inputs()
    assert 80 < (~k["vis"]).sum() < 120 and k["vis"][256:].any() and (~k["vis"][256:]).any()
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    sums, gm = dev(k["sums"]), dev(k["gm"])
    vis, radii = dev(k["vis"]), dev(k["radii"])
    acc, den, rad = (dev(a) for a in k["start"])
    use_s, use_m = variant in ("both", "no_g_means2d"), variant in ("both", "no_grad_sums")
    a = N.GsDensityStatsArgs(KN, KW, KH, N.ptr(vis), N.ptr(radii), N.ptr(sums) if use_s else None,
                             N.ptr(gm) if use_m else None, N.ptr(acc), N.ptr(den), N.ptr(rad))
    want = tuple(s.astype(np.float64) for s in k["start"])
    for step in range(2):  # two successive accumulations into non-zero starting values
        N.check(lib.gs_density_accumulate(C.byref(a), N.stream_ptr()), "gs_density_accumulate")
        want = _statement(*want, k["vis"], k["sums"] if use_s else None, k["gm"] if use_m else None, k["radii"], KW, KH)
    got = [_np(t) for t in (acc, den, rad)]
    inv = ~k["vis"]
    for g, s in zip(got, k["start"]):  # invisible rows keep their bits
        assert g[inv].tobytes() == s[inv].tobytes()
    assert np.array_equal(got[1].astype(np.float64), want[1])
    assert np.array_equal(got[2].astype(np.float64), want[2])
    rel = np.abs(got[0] - want[0]) / np.abs(want[0])
    print(f"grad_accum ({variant}): max rel err {rel.max():.3g}")
    # two products, a sum and a square root in fp32 stay within 3 ulp (3.6e-7); each accumulation rounds once
    assert rel.max() <= 1e-6
    if variant == "neither":
        assert np.array_equal(got[0], k["start"][0])  # the norm of nothing: + 0


def test_kernel_empty_and_single(pkg, cuda):
    N = pkg._native
    lib = N.load()
    assert lib.gs_density_accumulate(C.byref(N.GsDensityStatsArgs(n=0, image_width=8, image_height=8)),
                                     N.stream_ptr()) == 0
    st = pkg.DensityStats(1, cuda)
    vis, radii = torch.ones(1, dtype=torch.bool, device=cuda), torch.full((1,), 3.5, device=cuda)
    gm = torch.tensor([[3.0, 4.0]], device=cuda)
    a = N.GsDensityStatsArgs(1, 2, 2, N.ptr(vis), N.ptr(radii), None, N.ptr(gm), N.ptr(st.grad_accum), N.ptr(st.denom),
                             N.ptr(st.max_radii))
    N.check(lib.gs_density_accumulate(C.byref(a), N.stream_ptr()), "gs_density_accumulate")
    assert (st.grad_accum.item(), st.denom.item(), st.max_radii.item()) == (5.0, 1.0, 3.5)


# ---- end to end against the pinned oracle ----------------------------------------
def _ndc_norm(gxy, W, H):
    g = np.asarray(gxy, np.float64)
    return np.sqrt((0.5 * W * g[:, 0]) ** 2 + (0.5 * H * g[:, 1]) ** 2)


def _loss(out, f, dev):
    t = lambda k: FU.tensor(f[k], dev)
    L = (out["image"] * t("g_image")).sum() + (out["alpha"] * t("g_alpha")).sum() + (out["depth"] * t("g_depth")).sum()
    if "g_means2d" in f:
        L = L + (out["viewspace_points"] * t("g_means2d")).sum() + (out["conics"] * t("g_conics")).sum()
    return L


_TRUTH: dict = {}


def _truth(name):
    """The oracle's blend-only dL/dmeans2d of fixture `name` under the
    fixture's own cotangents, plus the fixture's cotangent on means2d where it
    has one, as the NDC-unit norm in fp64; and the oracle's vis and radii."""
    if name not in _TRUTH:
        f = G.load(name)
        H, W = int(f["height"]), int(f["width"])
        r = G.oracle().render_backward(G.scene_of(f), f["g_image"], f["g_alpha"], f["g_depth"])
        g = r["grads"]["means2d"].astype(np.float64)
        if "g_means2d" in f:
            g = g + np.asarray(f["g_means2d"], np.float64).reshape(-1, 2)
        vis = np.asarray(r["vis"], bool)
        _TRUTH[name] = (np.where(vis, _ndc_norm(g, W, H), 0.0), vis, np.where(vis, r["radii"], 0.0).astype(np.float32))
    return _TRUTH[name]


def _render_backward(pkg, dev, f, stats, frame_calls=None, budget=None):
    """One render + backward of the fixture's loss; the leaves' gradients."""
    RZ = pkg.rasterizer
    saved = RZ._FRAME_CALLS, RZ.PARTIAL_BUDGET_BYTES
    try:
        if frame_calls is not None:
            RZ._FRAME_CALLS = frame_calls
        if budget is not None:
            RZ.PARTIAL_BUDGET_BYTES = budget
        model, leaves, _ = FU.gaussians_of(pkg, dev, f)
        out = pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(FU.camera_of(f), model, FU.settings_of(pkg, f),
                                                                  density_stats=stats)
        _loss(out, f, dev).backward()
    finally:
        RZ._FRAME_CALLS, RZ.PARTIAL_BUDGET_BYTES = saved
    torch.cuda.synchronize()
    return out, {k: _np(t.grad) for k, t in leaves.items() if t.grad is not None}


E2E = [("offscreen", True, None), ("offscreen", False, None), ("model_random", True, None),
       ("model_random", False, None), ("tile12", None, None), ("tile32", None, None), ("tile32", None, 1),
       ("random_bg", None, None), ("tile8", None, None)]


@pytest.mark.parametrize("name,frame_calls,budget", E2E)
def test_statistics_match_the_oracle(pkg, cuda, name, frame_calls, budget):
    f = G.load(name)
    n = f["xyz"].shape[0]
    want, vis, radii = _truth(name)
    if name == "offscreen":
        assert vis.sum() == 18 and n == 24
    if budget is not None:  # one cell per batch: the batch_sums branch
        RZ = pkg.rasterizer
        cells = RZ.CameraParams(1, 1, 1, 1, 0, 0, (0,) * 12, (0, 0, 0), tile_size=int(f["tile"])).cells
        saved = RZ.PARTIAL_BUDGET_BYTES
        try:
            RZ.PARTIAL_BUDGET_BYTES = budget
            assert cells == 16 and RZ.cell_batch(cells, 1000) == 1
        finally:
            RZ.PARTIAL_BUDGET_BYTES = saved
    stats = pkg.DensityStats(n, cuda)
    out, grads = _render_backward(pkg, cuda, f, stats, frame_calls, budget)
    assert np.array_equal(_np(out["visibility_filter"]), vis)
    assert np.array_equal(_np(stats.denom), vis.astype(np.float32))
    assert np.array_equal(_np(stats.max_radii), np.where(vis, _np(out["radii"]), np.float32(0)))
    errs = G.check_grad("stats", _np(stats.grad_accum), want)
    assert want[vis].max() > 0 and not errs, errs
    # the same render without statistics: the same gradients, bit for bit
    _, plain = _render_backward(pkg, cuda, f, None, frame_calls, budget)
    assert plain.keys() == grads.keys() and len(grads) >= 4
    for k in grads:
        assert plain[k].tobytes() == grads[k].tobytes(), k
    # a second view adds to the first
    _render_backward(pkg, cuda, f, stats, frame_calls, budget)
    assert np.array_equal(_np(stats.denom), 2 * vis.astype(np.float32))
    assert not G.check_grad("stats x2", _np(stats.grad_accum), 2 * want)


@pytest.mark.parametrize("frame_calls", [True, False])
def test_nothing_visible_nothing_accumulated(pkg, cuda, frame_calls):
    f = G.load("all_behind")
    n = f["xyz"].shape[0]
    stats = pkg.DensityStats(n, cuda)
    RZ = pkg.rasterizer
    saved = RZ._FRAME_CALLS
    try:
        RZ._FRAME_CALLS = frame_calls
        model, leaves, _ = FU.gaussians_of(pkg, cuda, f)
        out = pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(FU.camera_of(f), model, FU.settings_of(pkg, f),
                                                                  density_stats=stats)
        out["viewspace_points"].sum().backward()
    finally:
        RZ._FRAME_CALLS = saved
    assert not out["visibility_filter"].any()
    for t in (stats.grad_accum, stats.denom, stats.max_radii):
        assert not t.any()


def test_no_blend_gradient_still_counts_views(pkg, cuda):
    """A backward with a cotangent on viewspace_points only: grad_sums is NULL,
    the statistic is the caller's cotangent's norm, views and radii count."""
    f = G.load("offscreen")
    n = f["xyz"].shape[0]
    H, W = int(f["height"]), int(f["width"])
    stats = pkg.DensityStats(n, cuda)
    model, _, _ = FU.gaussians_of(pkg, cuda, f)
    out = pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(FU.camera_of(f), model, FU.settings_of(pkg, f),
                                                              density_stats=stats)
    gm = np.random.default_rng(2).normal(0, 1, (n, 2)).astype(np.float32)
    (out["viewspace_points"] * FU.tensor(gm, cuda)).sum().backward()
    vis = _np(out["visibility_filter"])
    assert np.array_equal(_np(stats.denom), vis.astype(np.float32))
    assert np.array_equal(_np(stats.max_radii), np.where(vis, _np(out["radii"]), np.float32(0)))
    want = np.where(vis, _ndc_norm(gm, W, H), 0.0)
    assert np.abs(_np(stats.grad_accum) - want).max() <= 1e-6 * want.max()


def test_no_backward_no_statistics_and_retain_graph_counts_twice(pkg, cuda):
    f = G.load("offscreen")
    n = f["xyz"].shape[0]
    stats = pkg.DensityStats(n, cuda)
    model, _, _ = FU.gaussians_of(pkg, cuda, f)
    r = pkg.GaussianRenderer(**G.renderer_kwargs(f))
    with torch.no_grad():
        r.render(FU.camera_of(f), model, FU.settings_of(pkg, f), density_stats=stats)
    r.render(FU.camera_of(f), model, FU.settings_of(pkg, f), density_stats=stats)  # (its backward never runs)
    torch.cuda.synchronize()
    assert not stats.denom.any() and not stats.grad_accum.any() and not stats.max_radii.any()
    out = r.render(FU.camera_of(f), model, FU.settings_of(pkg, f), density_stats=stats)
    L = _loss(out, f, cuda)
    L.backward(retain_graph=True)
    once = stats.grad_accum.clone()
    L.backward()
    vis = _np(out["visibility_filter"])
    assert np.array_equal(_np(stats.denom), 2 * vis.astype(np.float32))
    assert torch.equal(stats.grad_accum, once + once)


def test_feature_pass_statistics(pkg, cuda):
    """C = 3 features, the cotangent on the feature image only: grad_sums is
    every feature chunk's geometry sums.  Truth: the oracle construction of
    features_util.oracle_features (one colour pass with color_logits =
    logit(F01), bg = 0, g_image = a gF, g_alpha = <b, gF>), its dL/dmeans2d."""
    f = G.load("zero_bg_tile12")
    n, c, seed = f["xyz"].shape[0], 3, 11
    H, W = int(f["height"]), int(f["width"])
    f01, a, b = FU.random_features(n, c, seed)
    gF = np.random.default_rng(seed + 1).uniform(-1, 1, (c, H, W)).astype(np.float32)
    sc = dataclasses.replace(G.scene_of(f), color_logits=np.log(f01 / (1 - f01)).astype(np.float32),
                             bg=np.zeros(3, np.float32))
    r = G.oracle().render_backward(sc, (a[:, None, None] * gF).astype(np.float32), np.tensordot(b, gF, 1),
                                   np.zeros((H, W)))
    vis = np.asarray(r["vis"], bool)
    want = np.where(vis, _ndc_norm(r["grads"]["means2d"], W, H), 0.0)
    stats = pkg.DensityStats(n, cuda)
    g = FU.Gauss(f["xyz"], f["cov3d"], f["color_logits"], f["opacity"], cuda)
    F = FU.tensor(a * f01 + b, cuda, grad=True)
    out = pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(FU.camera_of(f), g, FU.settings_of(pkg, f), features=F,
                                                              density_stats=stats)
    (out["features"] * FU.tensor(gF, cuda)).sum().backward()
    assert np.array_equal(_np(stats.denom), vis.astype(np.float32))
    assert np.array_equal(_np(stats.max_radii), np.where(vis, _np(out["radii"]), np.float32(0)))
    errs = G.check_grad("feature stats", _np(stats.grad_accum), want)
    assert want.max() > 0 and not errs, errs


def test_mismatched_statistics_are_refused(pkg, cuda):
    f = G.load("offscreen")
    n = f["xyz"].shape[0]
    model, _, _ = FU.gaussians_of(pkg, cuda, f)
    r = pkg.GaussianRenderer(**G.renderer_kwargs(f))
    bad = [pkg.DensityStats(n + 1, cuda), pkg.DensityStats(n, "cpu"), pkg.DensityStats(n, cuda), pkg.DensityStats(n, cuda)]
    bad[2].denom = bad[2].denom.double()
    bad[3].max_radii = torch.zeros(2 * n, device=cuda)[::2]
    for s in bad:
        with pytest.raises(ValueError, match="density_stats"):
            r.render(FU.camera_of(f), model, FU.settings_of(pkg, f), density_stats=s)
    # an empty model: nothing launched, nothing to add
    empty = FU.Gauss(np.zeros((0, 3)), np.zeros((0, 3, 3)), np.zeros((0, 3)), np.zeros(0), cuda)
    s0 = pkg.DensityStats(0, cuda)
    out = r.render(FU.camera_of(f), empty, FU.settings_of(pkg, f), density_stats=s0)
    out["viewspace_points"].sum().backward()
    assert s0.denom.numel() == 0


# ---- densification on the statistics ------------------------------------------------
def test_densify_on_statistics_matches_statement(pkg, cuda):
    n, th, ext, min_op, rmax, seed = 600, 2e-4, 1.0, 0.01, 20.0, 91
    m, _ = _model(pkg, cuda, n=n, seed=14)
    i = torch.arange(n)
    score_cls, rad_cls = i % 3, (i // 3) % 2          # score / th in {0 (no view), 0.5, 2}; radius / rmax in {0.5, 2}
    size_cls, dead = (i // 6) % 3, (i // 18) % 2      # the first 36 rows: every combination by construction
    with torch.no_grad():
        first = i < 36
        scl = torch.tensor([LARGE, SMALL, math.log(0.02)])[size_cls]
        m._scaling[first.to(cuda)] = scl[first, None].expand(-1, 3).to(cuda)
        m._opacity[first.to(cuda)] = torch.where(dead == 1, -10.0, 2.0)[first, None].to(cuda)
    # Adam moments to remap (the step moves the parameters: everything below reads them after it)
    opt = pkg.optim.FusedAdam([{"params": [p], "lr": 1e-3} for p in m.parameter_list()])
    for p in m.parameter_list():
        p.grad = torch.randn_like(p) * 1e-3
    opt.step()
    before = [(opt.state[p]["exp_avg"].clone(), opt.state[p]["exp_avg_sq"].clone()) for p in m.parameter_list()]
    denom = torch.where(score_cls == 0, 0.0, 1.0 + (i % 5).float())
    score = torch.tensor([0.0, 0.5, 2.0])[score_cls] * th
    accum = torch.where(score_cls == 0, torch.full((n,), 7.0), score * denom)  # (a sum nobody divides: score 0)
    radii = torch.tensor([0.5, 2.0])[rad_cls] * rmax
    stats = pkg.DensityStats(n, cuda)
    stats.grad_accum.copy_(accum), stats.denom.copy_(denom), stats.max_radii.copy_(radii)
    # the statement's gradient is the score (the fp32 quotient the kernel forms); no decision on a threshold
    q = torch.where(denom > 0, accum / denom.clamp_min(1), torch.zeros(n))
    assert torch.all((q == 0) | ((q / th - 0.5).abs() < 1e-3) | ((q / th - 2).abs() < 1e-3))
    grad = torch.stack([q, torch.zeros(n), torch.zeros(n)], -1).to(cuda)
    _make_safe(m, grad, th, ext, min_op)
    ref, (nk, ns, nc), (keep, sp, cl, hot, s, o) = ref_densify(m, grad, th, ext, min_op, seed, masks=True)
    big = radii.double() > rmax
    sizes = torch.where(s > 0.03 * ext, 0, torch.where(s < 0.01 * ext, 1, 2))
    combos = {(int(a), int(b), int(c), bool(d)) for a, b, c, d in zip(score_cls, rad_cls, sizes, o > min_op)}
    assert len(combos) == 36, "every (score, radius, size, opacity) combination"
    # the big rule on top of the statement: unsplit originals and their clones go, children stay
    sel = torch.cat([~big[keep], torch.ones(2 * ns, dtype=torch.bool), ~big[cl]])
    want = {k: v[sel] for k, v in ref.items()}
    keep2, cl2 = keep & ~big, cl & ~big
    assert min((keep & big).sum(), (cl & big).sum(), (sp & big).sum(), (sp & ~big).sum(), cl2.sum(), keep2.sum()) > 0
    with pytest.raises(ValueError, match="not both"):
        m.densify_and_prune(th, ext, min_op, seed=seed, xyz_grad=grad, stats=stats)
    info = m.densify_and_prune(th, ext, min_op, optimizer=opt, seed=seed, stats=stats, max_screen_radius=rmax)
    assert (info["kept"], info["split"], info["cloned"]) == (int(keep2.sum()), ns, int(cl2.sum()))
    assert info["n"] == info["kept"] + 2 * ns + info["cloned"] == m.get_num_points()
    got = dict(zip(NAMES, [p.detach().cpu().double() for p in m.parameter_list()]))
    for k in NAMES:
        assert got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        tol = 1e-4 if k == "op" else 1e-5  # (as tests/test_densify.py)
        err = (got[k] - want[k]).abs().max().item()
        assert err < tol, (k, err)
    kept = keep2.to(cuda)
    for p, (m0, v0) in zip(m.parameter_list(), before):
        st = opt.state[p]
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert torch.equal(st["exp_avg"][:info["kept"]], m0[kept]) and torch.equal(st["exp_avg_sq"][:info["kept"]], v0[kept])
        assert not st["exp_avg"][info["kept"]:].any() and not st["exp_avg_sq"][info["kept"]:].any()
    # the statistics restart as zeros of the new length
    assert m.density_stats.n == info["n"] and not m.density_stats.denom.any()
    # without the prune flag, or with max_screen_radius 0, the radius takes no part
    m2, _ = _model(pkg, cuda, n=n, seed=14)
    st2 = pkg.DensityStats(n, cuda)
    st2.max_radii.fill_(1e9)
    assert m2.densify_and_prune(th, ext, min_op, stats=st2, max_screen_radius=rmax, prune=False)["n"] == n
    m2.density_stats.max_radii.fill_(1e9)
    assert m2.densify_and_prune(th, ext, 0.0, stats=m2.density_stats, max_screen_radius=0.0)["n"] == n
