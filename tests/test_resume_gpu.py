"""A resumed run is the uninterrupted run, bit for bit, in every trainer mode.

Per mode three trainers on one dataset and config: A trains to END; B trains
to K and writes a checkpoint; C, a new trainer, loads it and trains the rest.
K lies inside a densification interval (tests/resume_util.py has the
schedule), where the state between steps is live: the "screen" criterion's
statistics, Adam moments over remapped rows, the 3D filter, the SH degree.
C's state right after the load equals B's, and C's state at END equals A's:
parameters, Adam moments and step counts, density statistics, filter state
and the counters, compared with torch.equal on the bit patterns.  There is no
tolerance in this file.

Each mode asserts what makes it sensitive (a densification before K, every
densification after K changing something, live statistics at K), and the two
statistic modes carry a control: Z, which is C with its statistics zeroed
after the load -- what load_checkpoint did before it stored them -- must
differ from A."""
import dataclasses
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import resume_util as RU
from resume_util import END, K, K_AT_DENSIFY
from scene_util import load_scene, write_scene_files
from test_density_training_gpu import _middle_threshold

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))

SCREEN = dict(densify_criterion="screen", prune_screen_radius=20.0)
XYZ = dict(densify_grad_threshold=2e-5)

# mode -> (config on top of resume_util.base_config, the checkpoint iteration)
MODES = {
    "xyz_grad": (XYZ, K),
    "screen": (SCREEN, K),
    "absgrad": (dict(SCREEN, densify_absgrad=True), K),
    # opacity resets at 17 (before K) and 34 (after): zeroed opacity moments under a kept step count.
    # opacity_lr: at the default 0.05 a capped opacity needs some 50 steps to come back, 3DGS resets
    # every 3000; with a dozen steps between reset and densification nothing is cloned after K at
    # any interval tried (3, 11, 12, 17), so the row could not tell a resumed run from another.  At
    # 0.5 the opacities recover in a few steps: 229 and 347 clones at 24 and 32
    "screen_reset": (dict(SCREEN, opacity_reset_interval=RU.RESET_INTERVAL, opacity_lr=0.5), K),
    "mcmc": ("mcmc", K),
    "filter3d": (dict(SCREEN, filter_3d=True, filter_3d_interval=RU.FILTER_INTERVAL), K),
    "visible_adam": (dict(SCREEN, visible_adam=True), K),
    # the degree rises at 15 (before K) and at 30 (after)
    "sh": (dict(XYZ, sh_degree=2, sh_increase_interval=RU.SH_INTERVAL), K),
    "distortion": (dict(XYZ, lambda_distortion=100.0, distortion_from_iter=K + 3), K),
    # at 0.01 (RadSplat's default) every one of the 13782 Gaussians of iteration K + 5 stays: the row
    # covers compact()'s renders and resets; at 0.05 it drops 2044 rows and their moments
    "contrib_prune": (dict(XYZ, contribution_prune_iterations=(K + 5,), contribution_prune_threshold=0.01), K),
    "contrib_prune_rows": (dict(XYZ, contribution_prune_iterations=(K + 5,), contribution_prune_threshold=0.05), K),
    "reset_adam": (dict(XYZ, reset_adam_on_densify=True), K),
    # a densification iteration itself: the optimizer was just rebuilt, the checkpoint has no adam.* key
    "reset_adam_at_densify": (dict(XYZ, reset_adam_on_densify=True), K_AT_DENSIFY),
}
CONTROLLED = ("screen", "absgrad")


@pytest.fixture(scope="module")
def scene(pkg, cuda, tmp_path_factory):
    root = tmp_path_factory.mktemp("resume_scene")
    write_scene_files(root, 12, 64)
    return root, load_scene(pkg, root, cuda, 64)


def _mcmc_config(pkg, out):
    """dp_mcmc_worker.mcmc_config's fields on this file's schedule; N grows
    2000 -> 2100 -> 2205 (K) -> 2315 -> 2400: the cap is reached at 32."""
    from dp_mcmc_worker import mcmc_config
    base = RU.base_config(pkg, out)
    keep = ("iterations", "densify_from_iter", "densify_until_iter", "densify_interval", "num_random_points",
            "log_interval", "output_path")
    return dataclasses.replace(mcmc_config(pkg, out), mcmc_cap_max=2400, **{k: getattr(base, k) for k in keep})


def _config(pkg, ds, mode, out):
    """The mode's config.  The screen modes' thresholds are inputs, chosen as
    tests/test_density_training_gpu.py chooses them: a calibration trainer of
    the same config runs to just before the first densification, and the
    thresholds are the middles of its statistics."""
    extra = MODES[mode][0]
    if extra == "mcmc":
        return _mcmc_config(pkg, out)
    cfg = RU.base_config(pkg, out, **extra)
    if cfg.densify_criterion == "screen":
        cal = pkg.GaussianTrainer(cfg, ds)
        cal.setup()
        cal.train(RU.FROM - 1)
        st = cal.gaussians.density_stats
        th = {"densify_grad_threshold": _middle_threshold(st.mean_grad(), st.denom)}
        if cfg.densify_absgrad:
            th["densify_abs_grad_threshold"] = _middle_threshold(st.mean_abs_grad(), st.denom)
        cfg = dataclasses.replace(cfg, **th)
    return cfg


def _changed(info):
    return info["relocated"] + info["added"] if "relocated" in info else info["split"] + info["cloned"]


def _run_a(pkg, ds, cfg, k):
    """The uninterrupted run; every densification after k changed something."""
    a = pkg.GaussianTrainer(cfg, ds)
    a.setup()
    seen = []
    for name in ("densify_and_prune", "relocate_and_grow"):  # (the trainer calls one of them every iteration)
        def spy(iteration, *args, _inner=getattr(a.optimizer, name), **kw):
            info = _inner(iteration, *args, **kw)
            if info is not None and iteration > k:
                seen.append((iteration, dict(info)))
            return info
        setattr(a.optimizer, name, spy)
    a.train(END)
    assert a.iteration == END and len(seen) >= 2, seen
    assert all(_changed(info) > 0 for _, info in seen), seen
    return a, seen


def _run_b(pkg, ds, cfg, k):
    b = pkg.GaussianTrainer(cfg, ds)
    b.setup()
    b.train(k)
    path = b.save_checkpoint(k)
    assert b.last_densify is not None, "no densification before the checkpoint"
    if cfg.densify_criterion == "screen":
        assert b.gaussians.density_stats.denom.any(), "the statistics are not live at the checkpoint"
    return b, path


def _resume(pkg, ds, cfg, k, zero_stats=False):
    c = pkg.GaussianTrainer(cfg, ds)
    c.load_checkpoint(k)
    at_load = RU.state(c)
    if zero_stats:
        c.gaussians.density_stats.reset()
    c.train(END - k)
    return c, at_load


@pytest.mark.parametrize("mode", list(MODES))
def test_resumed_run_equals_uninterrupted(pkg, cuda, scene, tmp_path, mode):
    _, ds = scene
    k = MODES[mode][1]
    cfg = _config(pkg, ds, mode, tmp_path / "out")
    a, densified = _run_a(pkg, ds, cfg, k)
    b, path = _run_b(pkg, ds, cfg, k)
    at_k = RU.state(b)
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        keys = set(f.keys())
    c, at_load = _resume(pkg, ds, cfg, k)
    want, got = RU.state(a), RU.state(c)
    print(f"{mode}: K = {k}, densifications after it {densified}; N {at_k['n']} -> {want['n']}; "
          f"{len(keys)} checkpoint keys; differences after the load {RU.differences(at_k, at_load)}, "
          f"at END {RU.differences(want, got)}")
    if mode == "reset_adam_at_densify":
        assert not [x for x in keys if x.startswith("adam.")] and not b.optimizer.optimizer.state
    if mode == "mcmc":
        assert at_k["n"] < cfg.mcmc_cap_max == want["n"], "the cap is to be reached after K only"
    if mode == "sh":
        assert (at_k["active_sh_degree"], want["active_sh_degree"]) == (1, 2)
        assert "adam.features_rest.m" in at_k and at_k["adam.features_rest.step"] < at_k["adam.xyz.step"]
    if mode == "screen_reset":
        assert at_k["adam.opacity.step"] == at_k["adam.xyz.step"]
    if mode.startswith("contrib_prune"):
        print(f"{mode}: contribution pruning {a.last_compact}")
        assert a.last_compact is not None and a.last_compact == c.last_compact
        if mode == "contrib_prune_rows":
            assert 0 < a.last_compact["n_after"] < a.last_compact["n_before"]
    RU.assert_same(at_k, at_load, f"{mode}: the state after load_checkpoint({k}) and the saved trainer's")
    RU.assert_same(want, got, f"{mode}: the resumed run and the uninterrupted one at {END}")
    if mode in CONTROLLED:
        # the control: the same resume with the statistics zeroed after the load must not be the same run
        z, _ = _resume(pkg, ds, cfg, k, zero_stats=True)
        bad = [x for x in RU.differences(want, RU.state(z)) if x in RU.PARAMS or x == "last_densify"]
        print(f"{mode}: with zeroed statistics the resumed run differs in {bad}")
        assert bad, "a resume without the statistics equals the uninterrupted run: the schedule is not sensitive"


def test_resume_in_a_fresh_process(pkg, cuda, scene, tmp_path):
    """The absgrad mode with C in a child process.  An in-process resume
    inherits the rasterizer's warm module state (the depth-key window history,
    the capacity guesses); a real one starts cold and takes the 32-bit-key and
    re-emission paths on its first frames.  The same bits."""
    root, ds = scene
    cfg = _config(pkg, ds, "absgrad", tmp_path / "out")
    a, _ = _run_a(pkg, ds, cfg, K)
    _run_b(pkg, ds, cfg, K)
    images = tmp_path / "images.npz"
    np.savez(images, images=torch.stack([c._image for c in ds.cameras]).cpu().numpy())
    out = tmp_path / "resumed.npz"
    rc = subprocess.run([sys.executable, os.path.join(HERE, "resume_worker.py"), str(root), str(images),
                         str(tmp_path / "out"), str(out), repr(cfg.densify_grad_threshold),
                         repr(cfg.densify_abs_grad_threshold)], timeout=240).returncode
    assert rc == 0, rc
    got = RU.state_from_numpy(np.load(out), cuda)
    RU.assert_same(RU.state(a), got, "the run resumed in a fresh process and the uninterrupted one")
