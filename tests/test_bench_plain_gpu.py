"""A plain bench.py run (no --full) at C1 with a few steps: the result line
carries the headline fields and none of the --full measurements, and
--dump-outputs writes the last timed step's outputs -- the frame the renderer
draws for the same seeded scene, and Adam's updated parameters."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_plain_run_line_and_dumped_outputs(pkg, cuda, tmp_path):
    import bench
    out = tmp_path / "dump"
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "1", "--config", "C1", "--steps", "6", "--warmup", "2",
                        "--spinup-steps", "3", "--dump-outputs", str(out)], cwd=ROOT, capture_output=True,
                       text=True, timeout=100)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1, p.stdout[-3000:]
    line = json.loads(lines[0])
    assert line["metric"] == bench.METRIC and line["unit"] == "Mpix/s" and line["higher_is_better"] is True
    assert line["dtype"] == "f32" and line["steps"] == 6 and line["full"] is False
    assert line["ms_per_step"] > 0
    n, W, H = bench.CONFIGS["C1"]
    assert line["value"] == pytest.approx(W * H / (line["ms_per_step"] * 1e-3) / 1e6, rel=1e-3)
    for k in ("stages_ms", "roofline", "cpu_baseline", "psnr_vs_ref"):
        assert k not in line
    assert line["graph"]["replayed"] is True and line["graph"]["steps_redone_in_timed_region"] == 0

    got = {f[:-4]: np.load(out / f) for f in sorted(os.listdir(out))}
    names = {"image", "alpha", "depth", "visibility_filter",
             "param_xyz", "param_features_dc", "param_opacity", "param_scaling", "param_rotation"}
    assert set(got) == names and set(line["dumped_outputs"]["arrays"]) == names
    assert all(v.dtype == np.float32 for v in got.values())
    assert sum(v.nbytes for v in got.values()) <= 64 << 20
    # the frame: the bench renders the same scene in every step (Adam writes to
    # shadow tensors), so it is the renderer's frame of the seeded scene
    scene = pkg.synthetic.make_scene(n, W, H, seed=0)
    model = pkg.synthetic.to_model(scene, pkg.GaussianModel, cuda)
    cam = bench.BenchCamera(W, H, scene.fovx, scene.fovy, bench.view_matrix(0))
    settings = pkg.RenderSettings(image_height=H, image_width=W, bg_color=torch.zeros(3))
    with torch.no_grad():
        ref = pkg.GaussianRenderer().render(cam, model, settings)
    for k in ("image", "alpha", "depth", "visibility_filter"):
        assert got[k].shape == tuple(ref[k].shape)
        assert np.array_equal(got[k], ref[k].to(torch.float32).cpu().numpy()), k
    # the parameters Adam wrote: finite, shaped like the model's, and one update
    # away from them (the model is never overwritten).  Every step sees the same
    # gradient, so |m_hat| / sqrt(v_hat) = 1 and an element moves by its learning
    # rate, 0.05 at most (opacity), or not at all (no gradient)
    for k, p in (("xyz", model._xyz), ("features_dc", model._features_dc), ("opacity", model._opacity),
                 ("scaling", model._scaling), ("rotation", model._rotation)):
        new, old = got["param_" + k], p.detach().cpu().numpy()
        assert new.shape == old.shape and np.isfinite(new).all()
        d = np.abs(new - old).max()
        assert 0 < d <= 0.06, (k, d)
