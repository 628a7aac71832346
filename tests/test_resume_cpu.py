"""GaussianTrainer.save_checkpoint / load_checkpoint on the CPU: what a
checkpoint holds per mode, and that a new trainer gets all of it back.  The
density statistics of the "screen" criterion are state between two
densifications (tests/test_resume_gpu.py trains across one); here they and the
Adam state are fabricated, so that no kernel is needed."""
from types import SimpleNamespace

import pytest
import torch

import resume_util as RU
from scene_util import write_scene_files

N = 37
ADAM_KEYS = {f"adam.{p}.{s}" for p in RU.PARAMS for s in ("m", "v", "step")}
BASE_KEYS = set(RU.PARAMS) | ADAM_KEYS
DENSITY3 = {"density.grad_accum", "density.denom", "density.max_radii"}
MODES = {
    "xyz_grad": (dict(), set()),
    "mcmc": (dict(densify_criterion="mcmc"), set()),
    "screen": (dict(densify_criterion="screen"), DENSITY3),
    "absgrad": (dict(densify_criterion="screen", densify_absgrad=True), DENSITY3 | {"density.abs_accum"}),
}


@pytest.fixture
def dataset(pkg, tmp_path):
    write_scene_files(tmp_path, 3, 8)  # (blank images: nothing here renders)
    ds = pkg.NeRFSyntheticDataset(str(tmp_path))
    ds.load_cameras()
    return ds


def _config(pkg, tmp_path, **kw):
    return pkg.TrainingConfig(device="cpu", num_random_points=N, output_path=str(tmp_path / "out"), **kw)


def _filled(pkg, ds, cfg, seed=5):
    """A trainer after setup() whose statistics hold seeded random values and
    whose parameters each have an Adam state with a step count of its own."""
    tr = pkg.GaussianTrainer(cfg, ds)
    tr.setup()
    assert tr.gaussians._xyz.device.type == "cpu" and tr.gaussians.get_num_points() == N
    g = torch.Generator().manual_seed(seed)
    st = tr.gaussians.density_stats
    assert (st.abs_accum is not None) == cfg.densify_absgrad
    for name in RU.STATS:
        t = getattr(st, name)
        if t is not None:
            t.copy_(torch.rand(N, generator=g) * (1 + torch.randint(0, 9, (N,), generator=g)))
    for i, p in enumerate(tr.gaussians.parameter_list()):
        tr.optimizer.optimizer.state[p] = {"step": 11 + i, "exp_avg": torch.randn(p.shape, generator=g),
                                           "exp_avg_sq": torch.rand(p.shape, generator=g)}
    tr.gaussians.active_sh_degree = 2
    tr.iteration = 7
    return tr


def _keys(path):
    from safetensors import safe_open
    with safe_open(path, framework="pt") as f:
        return set(f.keys())


def _without_density(state):
    return {k: v for k, v in state.items() if not k.startswith("density.")}


@pytest.mark.parametrize("mode", list(MODES))
def test_round_trip_and_key_set(pkg, dataset, tmp_path, mode):
    extra, density_keys = MODES[mode]
    cfg = _config(pkg, tmp_path, **extra)
    tr = _filled(pkg, dataset, cfg)
    tr.last_densify = {"kept": 30, "split": 3, "cloned": 1, "n": N}
    assert _keys(tr.save_checkpoint(7)) == BASE_KEYS | density_keys
    new = pkg.GaussianTrainer(cfg, dataset)
    new.load_checkpoint(7)
    assert new.gaussians._xyz.device.type == "cpu", "load_checkpoint ignored config.device"
    want, got = RU.state(tr), RU.state(new)
    assert {k for k in want if k.startswith("density.")} == (density_keys or DENSITY3)
    if density_keys:
        RU.assert_same(want, got, mode)
    else:  # not state in this mode: not written, zeros after the load
        RU.assert_same(_without_density(want), _without_density(got), mode)
        assert not any(got[k].any() for k in DENSITY3)
    assert got["iteration"] == 7 and got["active_sh_degree"] == 2 and got["adam.opacity.step"] == 16
    assert new._perm is not None and new.scene_extent == tr.scene_extent


def test_no_last_densify_and_no_adam_state(pkg, dataset, tmp_path):
    """Before the first step: no optimizer state, no densification."""
    cfg = _config(pkg, tmp_path, densify_criterion="screen")
    tr = pkg.GaussianTrainer(cfg, dataset)
    tr.setup()
    assert _keys(tr.save_checkpoint(0)) == set(RU.PARAMS) | DENSITY3
    new = pkg.GaussianTrainer(cfg, dataset)
    new.load_checkpoint(0)
    RU.assert_same(RU.state(tr), RU.state(new), "a fresh trainer")
    assert new.last_densify is None and not new.optimizer.optimizer.state


def test_checkpoint_without_statistics_loads_as_zeros(pkg, dataset, tmp_path):
    """An older checkpoint (or another criterion's) has no density.* key."""
    old = _filled(pkg, dataset, _config(pkg, tmp_path))
    assert _keys(old.save_checkpoint(7)) == BASE_KEYS
    new = pkg.GaussianTrainer(_config(pkg, tmp_path, densify_criterion="screen", densify_absgrad=True), dataset)
    new.load_checkpoint(7)
    got = RU.state(new)
    RU.assert_same(_without_density(RU.state(old)), _without_density(got), "everything but the statistics")
    assert all(got[f"density.{k}"].shape == (N,) and not got[f"density.{k}"].any() for k in RU.STATS)


def test_mismatched_absgrad(pkg, dataset, tmp_path):
    screen = dict(densify_criterion="screen")
    with_abs = _filled(pkg, dataset, _config(pkg, tmp_path / "a", densify_absgrad=True, **screen))
    with_abs.save_checkpoint(7)
    plain = pkg.GaussianTrainer(_config(pkg, tmp_path / "a", **screen), dataset)
    plain.load_checkpoint(7)  # the fourth buffer is ignored
    want, got = RU.state(with_abs), RU.state(plain)
    assert plain.gaussians.density_stats.abs_accum is None and "density.abs_accum" in want
    want.pop("density.abs_accum")
    RU.assert_same(want, got, "absgrad checkpoint, plain config")
    without = _filled(pkg, dataset, _config(pkg, tmp_path / "b", **screen))
    without.save_checkpoint(7)
    new = pkg.GaussianTrainer(_config(pkg, tmp_path / "b", densify_absgrad=True, **screen), dataset)
    new.load_checkpoint(7)  # the fourth buffer starts at zero
    got = RU.state(new)
    assert got["density.abs_accum"].shape == (N,) and not got.pop("density.abs_accum").any()
    RU.assert_same(RU.state(without), got, "plain checkpoint, absgrad config")


@pytest.mark.parametrize("bad", ["short", "long", "2d", "fp64"])
def test_statistics_of_another_shape_or_type_are_refused(pkg, dataset, tmp_path, bad):
    from safetensors.torch import load_file, save_file
    cfg = _config(pkg, tmp_path, densify_criterion="screen")
    path = _filled(pkg, dataset, cfg).save_checkpoint(7)
    t = load_file(path)
    d = t["density.denom"]
    t["density.denom"] = {"short": d[:-1].contiguous(), "long": torch.cat([d, d[:1]]), "2d": d[:, None].contiguous(),
                          "fp64": d.double()}[bad]
    save_file(t, path, metadata={"iteration": "7", "active_sh_degree": "0"})
    with pytest.raises(ValueError, match="density.denom"):
        pkg.GaussianTrainer(cfg, dataset).load_checkpoint(7)


def test_data_parallel_writes_and_reads_no_statistics(pkg, dataset, tmp_path):
    """Each rank's statistics are its own partial sums until the
    densification's all-reduce; one file cannot hold them."""
    group = SimpleNamespace(get_world_size=lambda: 2, get_rank=lambda: 0)
    cfg = _config(pkg, tmp_path, densify_criterion="screen", densify_absgrad=True)
    tr = _filled(pkg, dataset, cfg)
    single = tr.save_checkpoint(8)
    assert _keys(single) == BASE_KEYS | MODES["absgrad"][1]
    tr._dist = group
    assert _keys(tr.save_checkpoint(7)) == BASE_KEYS
    for it in (7, 8):  # neither its own file nor a single-process one gives a rank statistics
        new = pkg.GaussianTrainer(cfg, dataset)
        new._dist = group
        new.load_checkpoint(it)
        got = RU.state(new)
        assert new._dist is group and not any(got[f"density.{k}"].any() for k in RU.STATS)
        assert got.pop("iteration") == it
        want = _without_density(RU.state(tr))
        want.pop("iteration")
        RU.assert_same(want, _without_density(got), "everything but the statistics")
    one = SimpleNamespace(get_world_size=lambda: 1, get_rank=lambda: 0)  # a group of one rank is a single process
    tr._dist = one
    assert _keys(tr.save_checkpoint(9)) == BASE_KEYS | MODES["absgrad"][1]
