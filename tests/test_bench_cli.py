"""bench.py's argument handling (no GPU): presets, the workload name the
line carries, and the preset-dependent spin-up / timed-step defaults."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _parse(monkeypatch, *args):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *args])
    return bench.parse()


def test_presets_and_workload_names(monkeypatch):
    import bench
    a = _parse(monkeypatch)
    assert (a.config, a.gaussians, a.width, a.height) == ("C3", 1_000_000, 1920, 1080)
    assert (a.steps, a.spinup_steps) == (30, 50)  # the headline defaults
    assert bench.workload_name(a.gaussians, a.width, a.height) == "C3"
    a = _parse(monkeypatch, "--config", "C1")
    assert (a.gaussians, a.width, a.height, a.steps, a.spinup_steps) == (5_000, 256, 256, 500, 1000)
    assert bench.workload_name(a.gaussians, a.width, a.height) == "C1"
    a = _parse(monkeypatch, "--config", "C2", "--steps", "7", "--spinup-steps", "3", "--gaussians", "1234")
    assert (a.steps, a.spinup_steps, a.gaussians, a.width) == (7, 3, 1234, 800)
    assert bench.workload_name(a.gaussians, a.width, a.height) == "custom"
    for name, (n, w, h) in bench.CONFIGS.items():
        assert bench.workload_name(n, w, h) == name


def test_plain_run_is_the_default(monkeypatch):
    a = _parse(monkeypatch, "--gpus", "1", "--steps", "5", "--warmup", "2")
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (5, 2, False, None)
    a = _parse(monkeypatch, "--full", "--dump-outputs", "somewhere")
    assert a.full is True and a.dump_outputs == "somewhere"


def test_dump_arrays_whole_and_sampled(tmp_path):
    import numpy as np
    import torch
    import bench
    g = torch.Generator().manual_seed(3)
    arrays = {"image": torch.rand(3, 20, 30, generator=g), "vis": torch.rand(500, generator=g) > 0.5,
              "big": torch.rand(1000, 4, generator=g).double()}
    # within the budget: every array whole, in its shape, as float32
    shapes = bench.dump_arrays(str(tmp_path / "whole"), arrays, budget_bytes=4 * 6300)
    assert shapes == {"image": [3, 20, 30], "vis": [500], "big": [1000, 4]}
    for k, t in arrays.items():
        got = np.load(tmp_path / "whole" / f"{k}.npy")
        assert got.dtype == np.float32 and np.array_equal(got, t.to(torch.float32).numpy())
    # over it: arrays larger than an equal share are a sample of that size, the
    # same elements in every call, taken from the array in increasing index order
    budget = 4 * 3000
    s1 = bench.dump_arrays(str(tmp_path / "s1"), arrays, budget_bytes=budget)
    assert s1 == {"image": [1000], "vis": [500], "big": [1000]}
    other = {k: torch.rand(v.shape, generator=g).to(v.dtype) for k, v in arrays.items()}
    bench.dump_arrays(str(tmp_path / "s2"), other, budget_bytes=budget)
    total = 0
    for k, t in arrays.items():
        got = np.load(tmp_path / "s1" / f"{k}.npy")
        total += got.nbytes
        flat = t.to(torch.float32).numpy().reshape(-1)
        if got.size == flat.size:
            assert np.array_equal(got, flat)
            continue
        # the sampled indices, recovered from a second dump of index-valued data
        bench.dump_arrays(str(tmp_path / "idx"), {n: torch.arange(v.numel(), dtype=torch.float32).view(v.shape)
                                                   for n, v in arrays.items()}, budget_bytes=budget)
        idx = np.load(tmp_path / "idx" / f"{k}.npy").astype(np.int64)
        assert len(set(idx.tolist())) == idx.size and np.all(np.diff(idx) > 0)
        assert np.array_equal(got, flat[idx])
        assert np.array_equal(np.load(tmp_path / "s2" / f"{k}.npy"),
                              other[k].to(torch.float32).numpy().reshape(-1)[idx])
    assert total <= budget
