"""Per-Gaussian blend contribution statistics, the dominant-Gaussian maps and
contribution pruning on the GPU.  The reference for the weights is the feature
pass with features = eye(N): its image, already checked against the oracle
(tests/test_features_gpu.py), is Wt[g, p] = fma(c_g(p), 1, 0) plus exact
zeros = c_g(p).  That image comes from k_feat_fwd, a sibling of the kernels
under test; what pins it, and k_contrib and k_contrib_gather themselves, to
something independent is tests/test_replay_stage.py: every float against an
fp64 statement, not only the oracle at 1e-4."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import contrib_util as CU
import golden_io as G
from features_util import camera_of, gaussians_of, leaf_grad, settings_of, tensor
from scene_util import load_scene, write_scene_files
from stubs import Cam, Gauss
from test_dp_training_gpu import _free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

FIXTURES = ["kat_single", "kat_two_coaxial", "model_random", "saturate", "offscreen", "posed_camera", "tile8",
            "tile12", "tile32", "radius80_tile8", "all_behind"]

_CASES = {}


def _case(pkg, cuda, name):
    """The identity case of a fixture with fresh statistics: computed once,
    shared, never modified."""
    if name not in _CASES:
        _CASES[name] = CU.identity_case(pkg, cuda, G.load(name))
    return _CASES[name]


def second_camera(f):
    """The fixture's camera turned 0.12 rad about y and moved a little."""
    a = 0.12
    rot = np.array([[np.cos(a), 0, np.sin(a), 0.15], [0, 1, 0, -0.1], [-np.sin(a), 0, np.cos(a), 0.25], [0, 0, 0, 1]],
                   np.float32)
    return Cam(f["cam_width"], f["cam_height"], f["fovx"], f["fovy"], rot @ np.asarray(f["wv"], np.float32))


# ------------------------------------------------ 6: identity cross-check ----
def test_fixtures_are_small():
    for name in FIXTURES:
        f = G.load(name)
        assert f["xyz"].shape[0] <= 80 and int(f["width"]) <= 96 and int(f["height"]) <= 80, name


@pytest.mark.parametrize("name", FIXTURES)
def test_statistics_equal_the_feature_weights(pkg, cuda, name):
    f = G.load(name)
    r = _case(pkg, cuda, name)
    CU.check_against_weights(r, what=name)
    CU.check_sum(r["weight_sum"], r["Wt"], r["H"], r["W"], CU.tile_of(f), name)
    if name == "all_behind":
        assert not r["vis"].any() and (r["dom_id"] == -1).all() and not r["dom_w"].any()
    if name == "offscreen":
        assert (~r["vis"]).any(), "the fixture for culled rows has some"
    if name == "saturate":
        assert (r["alpha"] >= 0.995).any(), "the fixture for termination terminates somewhere"


@pytest.mark.parametrize("name", ["offscreen", "model_random", "all_behind"])
def test_prefilled_statistics_are_added_to(pkg, cuda, name):
    """A second statistics object with non-zero contents: seen rows are added
    to / maxed, culled rows keep their bits."""
    f = G.load(name)
    st = CU.prefilled(pkg, f["xyz"].shape[0], cuda)
    pre = CU.stats_arrays(st)
    r = CU.identity_case(pkg, cuda, f, stats=st)
    CU.check_against_weights(r, prefill=pre, what=name)
    seen = r["vis"]
    one = _case(pkg, cuda, name)["weight_sum"]  # (this view alone, from zero: 0 + s = s)
    assert np.array_equal(r["weight_sum"][seen], (pre["weight_sum"] + one)[seen])


# ------------------------------------------------ 7: against the colour pass ----
@pytest.mark.parametrize("name", ["model_random", "saturate", "tile12", "posed_camera"])
def test_weights_add_up_to_alpha(pkg, cuda, name):
    """alpha is the same c accumulated per pixel: both totals are fp32 sums of
    the same non-negative terms, each within (its longest chain) x 2^-24 of
    the exact total -- the Gaussians' chains as in test 6, a pixel's chain
    its list length (at most N entries)."""
    f = G.load(name)
    r = _case(pkg, cuda, name)
    n = r["Wt"].shape[0]
    exact = r["Wt"].astype(np.float64).sum()
    per_g = r["Wt"].astype(np.float64).sum(axis=1)
    b_stats = float((2.0 * CU.sum_chain(r["Wt"], r["H"], r["W"], CU.tile_of(f)) * CU.U24 * per_g).sum())
    b_alpha = 2.0 * n * CU.U24 * exact
    got, alpha = r["weight_sum"].astype(np.float64).sum(), r["alpha"].astype(np.float64).sum()
    print(f"  {name}: sum(weight_sum) {got:.9g}, sum(alpha) {alpha:.9g}, bound {b_stats + b_alpha:.3g}")
    assert exact > 0
    assert abs(got - alpha) <= b_stats + b_alpha


# ------------------------------------------------------ 8: accumulation ----
@pytest.mark.parametrize("name", ["model_random", "tile12"])
def test_two_cameras_accumulate(pkg, cuda, name):
    f = G.load(name)
    n = f["xyz"].shape[0]
    cam2 = second_camera(f)
    a = _case(pkg, cuda, name)
    b = CU.identity_case(pkg, cuda, f, camera=cam2)
    assert b["vis"].any() and not np.array_equal(a["weight_sum"], b["weight_sum"]), "a different view"
    CU.check_against_weights(b, what=name + " (second camera)")
    st = pkg.ContributionStats(n, cuda)
    CU.identity_case(pkg, cuda, f, stats=st)
    both = CU.identity_case(pkg, cuda, f, stats=st, camera=cam2)
    assert np.array_equal(both["weight_sum"], a["weight_sum"] + b["weight_sum"])  # (fp32 a + b)
    assert np.array_equal(both["weight_max"], np.maximum(a["weight_max"], b["weight_max"]))
    assert np.array_equal(both["pixels"], a["pixels"] + b["pixels"])
    assert np.array_equal(both["views"], a["views"] + b["views"])
    again = CU.identity_case(pkg, cuda, f)  # the same render twice: the same bits
    for k in ("weight_sum", "weight_max", "pixels", "views", "dom_id", "dom_w"):
        assert np.array_equal(a[k], again[k]), k


# ------------------------------------- 9: cell batches, no liveness bitmap ----
def _run_child(mode, path, env):
    subprocess.run([sys.executable, os.path.join(HERE, "contrib_util.py"), mode, path], check=True,
                   env=dict(os.environ, **env), timeout=300)
    return np.load(path)


def test_cell_batches(pkg, cuda, tmp_path):
    one = _case(pkg, cuda, "tile32")
    assert pkg.rasterizer.contribution_cell_batch(16, 10 ** 6) == 16, "the default budget: one batch"
    CU.identity_case(pkg, cuda, G.load("tile32"))  # (this frame's T is the device's last)
    T = int(pkg.rasterizer._T_SEEN[cuda])
    b = _run_child("batches", str(tmp_path / "batches.npz"), {"GS_PARTIAL_BUDGET": str(17 * T * 5 + 1)})
    assert int(b["T"]) == T and int(b["batch"]) == 5 and bool(b["same"])  # 5 + 5 + 5 + 1 cells
    for k in ("weight_max", "pixels", "views", "dom_id", "dom_w", "Wt"):
        assert np.array_equal(b[k], one[k]), k
    CU.check_sum(b["weight_sum"], one["Wt"], one["H"], one["W"], 32, "tile32 in batches of 5 cells")


def test_without_liveness_bitmap(pkg, cuda, tmp_path):
    one = _case(pkg, cuda, "tile32")
    b = _run_child("nolive", str(tmp_path / "nolive.npz"), {"GS_LIVE_BUDGET": "1"})
    assert bool(b["same"]) and int(b["batch"]) == 16
    for k in ("weight_sum", "weight_max", "pixels", "views", "dom_id", "dom_w", "Wt"):  # the extra entries add +0
        assert np.array_equal(b[k], one[k]), k


# ----------------------------------- 10: the training render is undisturbed ----
def test_training_render_undisturbed(pkg, cuda):
    f = G.load("model_random")
    assert "scaling" in f, "the raw-parameter path"
    n = f["xyz"].shape[0]
    H, W = int(f["height"]), int(f["width"])
    rng = np.random.default_rng(5)
    cot = {k: tensor(rng.uniform(-1, 1, s), cuda) for k, s in
           (("image", (3, H, W)), ("alpha", (1, H, W)), ("depth", (1, H, W)), ("viewspace_points", (n, 2)))}
    runs = []
    for with_stats in (False, True):
        model, leaves, _ = gaussians_of(pkg, cuda, f)
        ds = pkg.DensityStats(n, cuda)
        kw = dict(contribution_stats=pkg.ContributionStats(n, cuda), dominant=True) if with_stats else {}
        out = pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(camera_of(f), model, settings_of(pkg, f),
                                                                  density_stats=ds, **kw)
        sum((out[k] * c).sum() for k, c in cot.items()).backward()
        torch.cuda.synchronize()
        res = {k: out[k].detach().cpu().numpy() for k in ("image", "alpha", "depth", "viewspace_points",
                                                          "visibility_filter", "radii", "conics")}
        res.update({"d_" + k: leaf_grad(k, t, n) for k, t in leaves.items()})
        res.update(accum=ds.grad_accum.cpu().numpy(), denom=ds.denom.cpu().numpy(), radii_max=ds.max_radii.cpu().numpy())
        if with_stats:
            assert kw["contribution_stats"].views.any() and "dominant_gaussian" in out
        else:
            assert "dominant_gaussian" not in out and "dominant_weight" not in out
        runs.append(res)
    assert runs[0]["denom"].any() and np.abs(runs[0]["d_xyz"]).max() > 0
    for k in runs[0]:
        assert np.array_equal(runs[0][k], runs[1][k]), k


def test_combines_with_pose_filter_and_sh(pkg, cuda):
    """A differentiable pose, the screen filter and SH colour do not change
    what the weights are: the kernel replays whatever forward ran."""
    f = G.load("model_random")
    n = f["xyz"].shape[0]
    model = gaussians_of(pkg, cuda, f)[0]
    model.active_sh_degree = 2
    with torch.no_grad():
        model._features_rest.copy_(torch.randn(n, 15, 3, generator=torch.Generator().manual_seed(1)).to(cuda) * 0.1)
    wv = torch.tensor(np.asarray(f["wv"], np.float32), requires_grad=True)
    cam = camera_of(f)
    cam._wv = wv
    st = dataclasses.replace(settings_of(pkg, f), screen_filter=0.3)
    cs = pkg.ContributionStats(n, cuda)
    out = pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(cam, model, st, features=torch.eye(n, device=cuda),
                                                              contribution_stats=cs, dominant=True)
    out["image"].sum().backward()
    assert wv.grad is not None and torch.isfinite(wv.grad).all()
    H, W = int(f["height"]), int(f["width"])
    r = CU.stats_arrays(cs)
    r.update(Wt=out["features"].detach().cpu().numpy().reshape(n, H * W),
             dom_id=out["dominant_gaussian"].cpu().numpy().reshape(-1),
             dom_w=out["dominant_weight"].cpu().numpy().reshape(-1),
             vis=out["visibility_filter"].cpu().numpy().astype(bool))
    CU.check_against_weights(r, what="pose + filter + SH")
    CU.check_sum(r["weight_sum"], r["Wt"], H, W, CU.tile_of(f), "pose + filter + SH")


# ------------------------------------------------ 11: hidden Gaussians ----
class PrunableGauss(Gauss):
    """The cov3d stub with what GaussianOptimizer.prune_by_contribution asks of a model."""

    @property
    def _xyz(self):
        return self.xyz

    def get_num_points(self):
        return int(self.xyz.shape[0])

    def prune_points(self, mask, optimizer=None):
        for k in ("xyz", "cov", "feats", "op"):
            setattr(self, k, getattr(self, k).detach()[mask].contiguous().requires_grad_())


def _hidden_render(pkg, cuda, f, g, stats=None):
    kw = {} if stats is None else {"contribution_stats": stats}
    with torch.no_grad():
        out = pkg.GaussianRenderer(**G.renderer_kwargs(f)).render(camera_of(f), g, settings_of(pkg, f), **kw)
    return {k: out[k].cpu().numpy() for k in ("image", "alpha", "depth", "visibility_filter")}


@pytest.mark.parametrize("tile", [16, 8, 64])
def test_hidden_gaussians_are_found_and_pruned(pkg, cuda, tile):
    f = CU.hidden_scene(tile)
    hidden = np.array([0, 0, 0, 1, 1], bool)

    def fresh():
        return PrunableGauss(f["xyz"], f["cov3d"], f["color_logits"], f["opacity"], cuda)

    g = fresh()
    st = pkg.ContributionStats(5, cuda)
    before = _hidden_render(pkg, cuda, f, g, st)
    assert before["visibility_filter"].all(), "the hidden two are visible"
    wmax, pixels = st.weight_max.cpu().numpy(), st.pixels.cpu().numpy()
    assert (pixels[hidden] == 0).all() and (wmax[hidden] == 0).all()
    assert (pixels[~hidden] > 0).all() and (wmax[~hidden] > 0).all()
    opt = pkg.optim.GaussianOptimizer(g, pkg.TrainingConfig())
    assert opt.prune_by_contribution(st, 0.0) == {"n_before": 5, "n_after": 3}
    assert np.array_equal(g.xyz.detach().cpu().numpy(), f["xyz"][~hidden])
    after = _hidden_render(pkg, cuda, f, g)
    for k in ("image", "alpha", "depth"):
        assert np.array_equal(before[k], after[k]), k
    # a threshold between two observed values keeps exactly weight_max > t
    v = np.unique(wmax[wmax > 0])
    assert len(v) >= 2
    for lo, hi in zip(v[:-1], v[1:]):
        t = float((np.float64(lo) + np.float64(hi)) / 2)
        g2 = fresh()
        info = pkg.optim.GaussianOptimizer(g2, pkg.TrainingConfig()).prune_by_contribution(st, t)
        keep = wmax > np.float32(t)
        assert info == {"n_before": 5, "n_after": int(keep.sum())} and 0 < keep.sum() < 3
        assert np.array_equal(g2.xyz.detach().cpu().numpy(), f["xyz"][keep])


# ------------------------------------------------------ 12, 13: trainer ----
_config = CU.trainer_config


@pytest.fixture(scope="module")
def scene(pkg, cuda, tmp_path_factory):
    root = tmp_path_factory.mktemp("contrib_scene")
    write_scene_files(root, 8, 64)
    return root, load_scene(pkg, root, cuda, 64, split=False)


def _accumulate(tr):
    st = tr.gaussians.contribution_stats
    st.reset()
    with torch.no_grad():
        for cam in tr.dataset.get_train_cameras():
            tr.renderer.render(cam, tr.gaussians, tr._settings(cam), contribution_stats=st)
    return st


def _middle(wmax):
    """The midpoint of the two middle positive values: about half is pruned
    and no decision sits on the threshold."""
    v = np.unique(wmax[wmax > 0])
    assert len(v) >= 2
    return float((np.float64(v[len(v) // 2 - 1]) + np.float64(v[len(v) // 2])) / 2)


def test_moments_follow_the_kept_gaussians(pkg, cuda, scene, tmp_path):
    root, ds = scene
    cfg = _config(pkg, tmp_path / "a")
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    tr.train(3)
    st = _accumulate(tr)
    t = _middle(st.weight_max.cpu().numpy())
    keep = st.weight_max > t
    g, adam = tr.gaussians, tr.optimizer.optimizer
    # a fresh model of the kept rows, carrying their moments and step counts
    tr2 = pkg.GaussianTrainer(_config(pkg, tmp_path / "b"), ds)
    tr2.setup()
    tr2.gaussians._set(*[p.detach()[keep].clone() for p in g.parameter_list()])
    tr2.optimizer.setup_optimizer()
    stepped = 0
    for p, q in zip(g.parameter_list(), tr2.gaussians.parameter_list()):
        s = adam.state.get(p)
        if s:
            stepped += 1
            assert s["step"] == 3
            tr2.optimizer.optimizer.state[q] = {"step": s["step"], "exp_avg": s["exp_avg"][keep].clone(),
                                                "exp_avg_sq": s["exp_avg_sq"][keep].clone()}
    assert stepped == 5
    tr2.iteration = tr.iteration
    info = tr.optimizer.prune_by_contribution(st, t)
    n_keep = int(keep.sum())
    assert info == {"n_before": 3000, "n_after": n_keep} and 0 < n_keep < 3000
    assert g.contribution_stats.n == n_keep and not g.contribution_stats.views.any()
    for x in (tr, tr2):
        x.iteration += 1
        loss = x.train_step(x._camera_for(x.iteration))["loss"]
        assert torch.isfinite(loss)
    for p, q in zip(g.parameter_list(), tr2.gaussians.parameter_list()):
        assert torch.equal(p.detach(), q.detach())
        s, s2 = adam.state.get(p), tr2.optimizer.optimizer.state.get(q)
        assert bool(s) == bool(s2)
        if s:
            assert s["step"] == s2["step"] == 4
            assert torch.equal(s["exp_avg"], s2["exp_avg"]) and torch.equal(s["exp_avg_sq"], s2["exp_avg_sq"])


def test_trainer_compacts_on_schedule(pkg, cuda, scene, tmp_path):
    root, ds = scene
    k = 6

    def run(cfg, iterations, watch=False):
        tr = pkg.GaussianTrainer(cfg, ds)
        tr.setup()
        calls = []
        inner = tr.compact

        def compact(*a, **kw):
            calls.append((tr.iteration, tr.gaussians.get_num_points()))
            return inner(*a, **kw)

        tr.compact = compact
        sizes = []
        for _ in range(iterations):
            tr.train(1)
            sizes.append(tr.gaussians.get_num_points())
        torch.cuda.synchronize()
        return tr, calls, sizes

    # the threshold: from the statistics a default run holds at iteration k
    base, calls, _ = run(_config(pkg, tmp_path / "base"), k)
    assert calls == [] and base.last_compact is None
    t = _middle(_accumulate(base).weight_max.cpu().numpy())
    exp_keep = int((base.gaussians.contribution_stats.weight_max > t).sum())
    tr, calls, sizes = run(_config(pkg, tmp_path / "prune", contribution_prune_iterations=(k,),
                                   contribution_prune_threshold=t), 12)
    assert calls == [(k, 3000)], "compact() once, at iteration k, after the optimizer step"
    assert tr.last_compact == {"n_before": 3000, "n_after": exp_keep} and 0 < exp_keep < 3000
    assert sizes == [3000] * (k - 1) + [exp_keep] * (12 - k + 1), "N does not grow"
    assert tr.iteration == 12 and len(tr.train_losses) == 12 and np.isfinite(tr.train_losses).all()
    st = tr.gaussians.contribution_stats
    assert st.n == exp_keep and not st.views.any() and not st.weight_max.any()
    for p in tr.gaussians.parameter_list():
        assert p.shape[0] == exp_keep and torch.isfinite(p).all()
    # the default empty tuple: the run of a config that never names the new fields, bit for bit
    default, calls_d, _ = run(_config(pkg, tmp_path / "d"), 12)
    named, calls_n, _ = run(_config(pkg, tmp_path / "n", contribution_prune_iterations=(),
                                    contribution_prune_threshold=0.5), 12)
    assert calls_d == [] and calls_n == []
    for p, q in zip(default.gaussians.parameter_list(), named.gaussians.parameter_list()):
        assert torch.equal(p.detach(), q.detach())
    assert default.gaussians._contribution_stats is None, "no statistics were made, no launch added"


# --------------------------------------------------------- 14: two ranks ----
def test_two_ranks_compact_alike(pkg, cuda, scene, tmp_path):
    root, ds = scene
    cfg = _config(pkg, tmp_path / "single")
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    xyz0 = tr.gaussians._xyz.detach().cpu().numpy().copy()
    wmax = _accumulate(tr).weight_max.cpu().numpy()
    t = _middle(wmax)
    info = tr.compact(t)
    kept = np.nonzero(wmax > np.float32(t))[0]
    assert info == {"n_before": 3000, "n_after": len(kept)} and 0 < len(kept) < 3000
    single = tr.gaussians._xyz.detach().cpu().numpy()
    assert np.array_equal(single, xyz0[kept])
    port = _free_port()
    outs = [tmp_path / f"rank{r}.npz" for r in range(2)]
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dp_contrib_worker.py"), str(r), "2", str(port),
                               str(root), str(outs[r]), repr(t)], env=dict(os.environ, MASTER_ADDR="127.0.0.1"))
             for r in range(2)]
    try:
        rcs = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0, 0], rcs
    for o in outs:
        z = np.load(o)
        assert np.array_equal(z["xyz0"], xyz0), "the ranks start from the single process's model"
        assert int(z["n_before"]) == 3000 and int(z["n_after"]) == len(kept)
        assert np.array_equal(z["xyz"], single), "the kept index set"
        assert int(z["cameras"]) == 4, "each rank rendered its half of the cameras"
