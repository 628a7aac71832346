"""GaussianTrainer with densify_criterion = "screen": density control on the
statistics the renders' backwards accumulate -- one process, and two
data-parallel ranks whose statistics are all-reduced at the densification."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from dp_density_worker import screen_config
from scene_util import load_scene, write_scene_files
from test_dp_training_gpu import _free_port

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


def _middle_threshold(mean_grad, denom):
    """The midpoint of the two middle values of the seen Gaussians' mean
    gradient: an input chosen so that densification acts on about half of them
    and no decision sits on the threshold."""
    v = torch.sort(mean_grad[denom > 0].double().cpu()).values
    assert v.numel() >= 2 and v[v.numel() // 2 - 1] < v[v.numel() // 2]
    return float((v[v.numel() // 2 - 1] + v[v.numel() // 2]) / 2)


def test_trainer_densifies_on_screen_statistics(pkg, cuda, tmp_path):
    write_scene_files(tmp_path, 12, 64)
    ds = load_scene(pkg, tmp_path, cuda, 64)
    cfg = pkg.TrainingConfig(iterations=300, densify_from_iter=100, densify_until_iter=300, densify_interval=100,
                             num_random_points=3000, log_interval=100, output_path=str(tmp_path / "out"),
                             position_lr_init=1.6e-3, position_lr_final=1.6e-5, densify_criterion="screen",
                             opacity_reset_interval=200, prune_screen_radius=20.0)
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    before = tr.validate()
    st = tr.gaussians.density_stats
    assert st.n == 3000 and not st.denom.any(), "validate() adds nothing to the statistics"
    tr.train(99)
    assert tr.last_densify is None and st is tr.gaussians.density_stats
    seen = int((st.denom > 0).sum())
    assert seen > 100 and float(st.denom.max()) <= 99 and float(st.max_radii.max()) > 0
    cfg.densify_grad_threshold = _middle_threshold(st.mean_grad(), st.denom)
    tr.train(1)
    first = dict(tr.last_densify)
    print(f"threshold {cfg.densify_grad_threshold:.3g} ({seen} of 3000 seen): first densification {first}")
    assert first["split"] + first["cloned"] > 0
    assert tr.gaussians.density_stats.n == first["n"] and not tr.gaussians.density_stats.denom.any()
    tr.train(99)
    assert tr.gaussians.density_stats.denom.any()
    tr.train(1)  # iteration 200: densification, then the opacity reset
    cap = torch.tensor(np.log(0.01 / 0.99), dtype=torch.float32)
    assert float(tr.gaussians._opacity.detach().max()) <= float(cap)
    op_state = tr.optimizer.optimizer.state.get(tr.gaussians._opacity)
    assert op_state is None or (not op_state["exp_avg"].any() and not op_state["exp_avg_sq"].any())
    tr.train(100)
    assert tr.iteration == 300
    n = tr.gaussians.get_num_points()
    s = tr.gaussians.density_stats
    assert tr.last_densify["n"] == n == s.n
    for t in (s.grad_accum, s.denom, s.max_radii):
        assert t.shape == (n,) and not t.any()
    for p in tr.gaussians.parameter_list():
        assert torch.isfinite(p).all()
    after = tr.validate()
    print(f"PSNR {before['psnr']:.2f} -> {after['psnr']:.2f} dB; Gaussians 3000 -> {n}")
    assert after["psnr"] > before["psnr"]


def _two_rank_statement(pkg, ds, cfg, world, stop_before_densify=False):
    """One process: per iteration the views the ranks would render, one
    DensityStats per simulated rank, their gradients' mean, the same Adam
    step; at the densification the ranks' statistics are added (a + b, as the
    all-reduce adds them; max for the radii)."""
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    cams = ds.get_train_cameras()
    g = tr.gaussians
    per_rank = [pkg.DensityStats(g.get_num_points(), g._xyz.device) for _ in range(world)]
    for it in range(1, cfg.iterations + 1):
        tr.iteration = it
        if per_rank[0].n != g.get_num_points():
            per_rank = [pkg.DensityStats(g.get_num_points(), g._xyz.device) for _ in range(world)]
        grads = []
        for r in range(world):
            cam = cams[int(tr._perm[(it * world + r) % len(cams)])]
            tr.optimizer.zero_grad()
            out = tr.renderer.render(cam, g, tr._settings(cam), density_stats=per_rank[r])
            pkg.loss.photometric_loss(out["image"], cam._image, cfg.lambda_dssim)[0].backward()
            grads.append([p.grad.clone() for p in g.grad_parameters()])
        for i, p in enumerate(g.grad_parameters()):
            s = grads[0][i].clone()
            for k in range(1, world):
                s += grads[k][i]
            p.grad = s / world
        tr.optimizer.update_learning_rate(it)
        tr.optimizer.step()
        if tr.optimizer.density_controller.should_densify(it):
            total = g.density_stats
            total.grad_accum.copy_(per_rank[0].grad_accum + per_rank[1].grad_accum)
            total.denom.copy_(per_rank[0].denom + per_rank[1].denom)
            total.max_radii.copy_(torch.maximum(per_rank[0].max_radii, per_rank[1].max_radii))
            if stop_before_densify:
                return tr
        tr.last_densify = tr.optimizer.densify_and_prune(it, tr.scene_extent) or tr.last_densify
    return tr


def test_dp_two_ranks_densify_on_all_reduced_statistics(pkg, cuda, tmp_path):
    write_scene_files(tmp_path)
    ds = load_scene(pkg, tmp_path, cuda, split=False)
    # the threshold: from a single-process pre-run up to the densification
    pre = _two_rank_statement(pkg, ds, screen_config(pkg, tmp_path / "pre", 1.0), 2, stop_before_densify=True)
    st = pre.gaussians.density_stats
    assert float(st.denom.max()) == 4.0  # two ranks, two iterations
    threshold = _middle_threshold(st.mean_grad(), st.denom)
    port = _free_port()
    outs = [tmp_path / f"rank{r}.npz" for r in range(2)]
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", GS_ALLREDUCE_CHUNKS="2", GS_ALLREDUCE_MIN_ROWS="256")
    procs = [subprocess.Popen([sys.executable, os.path.join(HERE, "dp_density_worker.py"), str(r), "2", str(port),
                               str(tmp_path), str(outs[r]), repr(threshold)], env=env) for r in range(2)]
    try:
        rcs = [p.wait(timeout=240) for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    assert rcs == [0, 0], rcs
    a, b = (np.load(o) for o in outs)
    n0 = screen_config(pkg, tmp_path, threshold).num_random_points
    print(f"DP screen criterion, threshold {threshold:.3g}: {n0} -> {int(a['n'])} Gaussians "
          f"(split {int(a['split'])}, cloned {int(a['cloned'])})")
    assert int(a["iteration"]) == 3 and int(a["n"]) == int(b["n"]) != n0
    for i in range(6):
        assert np.array_equal(a[f"p{i}"], b[f"p{i}"]), f"replicas diverged in parameter {i}"
    ref = _two_rank_statement(pkg, ds, screen_config(pkg, tmp_path / "ref", threshold), 2)
    assert ref.gaussians.get_num_points() == int(a["n"])
    assert (ref.last_densify["split"], ref.last_densify["cloned"]) == (int(a["split"]), int(a["cloned"]))
    for i, p in enumerate(ref.gaussians.parameter_list()):
        assert np.array_equal(p.detach().cpu().numpy(), a[f"p{i}"]), f"DP step != two-rank statement (parameter {i})"
    # after the densification each rank's statistics hold its own view of iteration 3 only
    assert a["denom"].shape == (int(a["n"]),) and a["denom"].max() == 1.0 and b["denom"].max() == 1.0
    assert not np.array_equal(a["accum"], b["accum"])
